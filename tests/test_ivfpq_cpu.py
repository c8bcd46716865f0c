"""CPU: the IVF index over PQ codes (mi_ivfpq_*) is exported and bound, answers bad arguments before touching a device, the numpy
truth (tests/_ivfpq_truth.py) reduces to pq_truth when every list is probed and to what the reference's matching_PQ_Net_bucket
computes when one bucket is, and IVFPQIndex / matching_PQ_Net_bucket_hip reject bad input with ValueError before the device."""
import ctypes as C

import numpy as np
import pytest

from _ivfpq_truth import ivfpq_truth, probe_truth
from _pq_truth import dtable64, pq_truth

NEW = {"mi_ivfpq_create": 15, "mi_ivfpq_append_codes": 6, "mi_ivfpq_add": 7, "mi_ivfpq_probe": 8, "mi_ivfpq_search": 14,
       "mi_ivfpq_search_device": 10, "mi_ivfpq_info": 10, "mi_ivfpq_list_sizes": 2, "mi_ivfpq_get_rows": 5, "mi_ivfpq_destroy": 1}


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__
    __graft_entry__.build()
    from isehr_amd import _lib
    return _lib.load(), _lib


def test_symbols_are_exported_and_bound(built_lib):
    lib, _lib = built_lib
    for name, nargs in NEW.items():
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name).restype == C.c_int
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
    for meth in ("from_codes", "from_device_ptr", "empty", "fit", "append_codes", "add", "add_device", "probe", "search", "search_device",
                 "list_sizes", "get_rows", "hbm_bytes", "close", "__enter__", "__exit__"):
        assert hasattr(_lib.IVFPQIndex, meth), meth
    from isehr_amd import nnsearch
    assert callable(nnsearch.matching_PQ_Net_bucket_hip)
    assert nnsearch.matching_PQ_Net_bucket_hip not in nnsearch.MATCHING_METHODS.values()
    assert lib.mi_ivfpq_destroy(None) == 0


def test_invalid_arguments_answer_without_a_device(built_lib):
    lib, _lib = built_lib
    P = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    rng = np.random.default_rng(0)
    cb = rng.standard_normal((4, 16, 2)).astype(np.float32)                 # m = 4, ks = 16, L = 2, d = 8
    G = rng.standard_normal((5, 8)).astype(np.float32)                      # nlist = 5
    big = np.zeros(257 * 4100, np.float32)                                  # centroids / codebooks for the out-of-range shapes
    codes = np.zeros((3, 4), np.uint8)
    lists = np.zeros(3, np.uint8)
    h = C.c_void_p()

    def create(gp=None, nlist=5, cbp=None, d=8, m=4, ks=16, cd=P(codes), li=P(lists), n=3, stride=4, cap=0, out=C.byref(h)):
        return lib.mi_ivfpq_create(P(G) if gp is None else gp, nlist, P(cb) if cbp is None else cbp, d, m, ks, cd, li, n, stride,
                                   _lib.MI_HOST, 0, 0, cap, out)

    cases = [(dict(out=None), b"out"), (dict(nlist=1), b"nlist (lists)"), (dict(nlist=257, gp=P(big)), b"nlist (lists)"),
             (dict(m=0, cbp=P(big)), b"m (books)"), (dict(m=65, d=130, cbp=P(big), gp=P(big)), b"m (books)"),
             (dict(ks=1), b"ks (codewords"), (dict(ks=257, cbp=P(big)), b"ks (codewords"),
             (dict(d=9, cbp=P(big), gp=P(big)), b"multiple of m"), (dict(d=4100, cbp=P(big), gp=P(big)), b"d must be in"),
             (dict(d=0), b"d must be in"), (dict(cap=2), b"capacity"), (dict(cap=-1), b"capacity"),
             (dict(n=-1), b"negative number of rows"), (dict(cd=None), b"codes"), (dict(li=None), b"list_ids"),
             (dict(cd=None, li=None, n=0), b"capacity"), (dict(stride=3), b"row_stride_bytes")]
    for kwargs, word in cases:
        assert create(**kwargs) == _lib.MI_ERR_INVALID, kwargs
        assert word in lib.mi_last_error(), (kwargs, lib.mi_last_error())
    assert lib.mi_ivfpq_create(None, 5, P(cb), 8, 4, 16, P(codes), P(lists), 3, 4, _lib.MI_HOST, 0, 0, 0, C.byref(h)) == _lib.MI_ERR_INVALID
    assert b"coarse_host" in lib.mi_last_error()
    assert lib.mi_ivfpq_create(P(G), 5, None, 8, 4, 16, P(codes), P(lists), 3, 4, _lib.MI_HOST, 0, 0, 0, C.byref(h)) == _lib.MI_ERR_INVALID
    assert b"codebooks_host" in lib.mi_last_error()
    for bad_value in (np.nan, np.inf):
        bad_G = G.copy()
        bad_G[4, 7] = bad_value
        assert create(gp=P(bad_G)) == _lib.MI_ERR_INVALID
        assert b"coarse centroids must be finite" in lib.mi_last_error()
        bad_cb = cb.copy()
        bad_cb[3, 15, 1] = bad_value
        assert create(cbp=P(bad_cb)) == _lib.MI_ERR_INVALID
        assert b"codebooks must be finite" in lib.mi_last_error()
    bad_codes = codes.copy()
    bad_codes[2, 3] = 16
    assert create(cd=P(bad_codes)) == _lib.MI_ERR_INVALID
    assert b">= ks" in lib.mi_last_error()
    bad_lists = lists.copy()
    bad_lists[2] = 5
    assert create(li=P(bad_lists)) == _lib.MI_ERR_INVALID
    assert b">= nlist" in lib.mi_last_error()
    assert h.value is None

    q = np.zeros((2, 8), np.float32)
    idx = np.zeros(8, np.int64)
    pr = np.zeros((2, 3), np.int32)
    fake = C.c_void_p(16)                         # non-null, never dereferenced: these checks answer before the handle is read

    def search(hh=fake, k=4, nq=2, nprobe=3, probes=None, qp=P(q), out=P(idx)):
        return lib.mi_ivfpq_search(hh, qp, nq, _lib.MI_F32, 8, 1, k, nprobe, probes, None, _lib.MI_HOST, out, None, None)

    def search_dev(hh=fake, k=4, nq=2, nprobe=3, qp=P(q), out=P(idx)):
        return lib.mi_ivfpq_search_device(hh, qp, nq, k, nprobe, None, None, out, None, None)

    def probe(hh=fake, nq=2, nprobe=3, qp=P(q), out=P(pr)):
        return lib.mi_ivfpq_probe(hh, qp, nq, _lib.MI_F32, 8, 1, nprobe, out)

    common = [(dict(hh=None), b"null handle"), (dict(nq=-1), b"nq must"), (dict(nprobe=0), b"nprobe must"),
              (dict(nprobe=257), b"nprobe must"), (dict(qp=None), b"null pointer"), (dict(out=None), b"null pointer")]
    for fn in (search, search_dev, probe):
        for kwargs, word in common + ([] if fn is probe else [(dict(k=0), b"k must"), (dict(k=2049), b"k must")]):
            assert fn(**kwargs) == _lib.MI_ERR_INVALID, (fn.__name__, kwargs)
            assert word in lib.mi_last_error(), (fn.__name__, kwargs, lib.mi_last_error())
    # a host probe entry below -1, and one no index can hold (nlist <= 256): answered before the handle is read.  An entry of
    # exactly nlist needs the handle and is in tests/test_gpu_ivfpq.py; the wrapper's ValueError for it is below
    for bad in (-2, 256):
        bad_pr = pr.copy()
        bad_pr[1, 2] = bad
        assert search(probes=P(bad_pr)) == _lib.MI_ERR_INVALID
        assert b"probe entry" in lib.mi_last_error()
    assert lib.mi_ivfpq_append_codes(None, P(codes), P(lists), 3, 4, _lib.MI_HOST) == _lib.MI_ERR_INVALID
    assert lib.mi_ivfpq_append_codes(fake, P(codes), None, 3, 4, _lib.MI_HOST) == _lib.MI_ERR_INVALID
    assert b"list_ids" in lib.mi_last_error()
    assert lib.mi_ivfpq_append_codes(fake, None, P(lists), 3, 4, _lib.MI_HOST) == _lib.MI_ERR_INVALID
    assert lib.mi_ivfpq_append_codes(fake, P(codes), P(lists), -1, 4, _lib.MI_HOST) == _lib.MI_ERR_INVALID
    assert lib.mi_ivfpq_add(None, P(q), 2, _lib.MI_F32, 8, 1, _lib.MI_HOST) == _lib.MI_ERR_INVALID
    assert lib.mi_ivfpq_add(fake, None, 2, _lib.MI_F32, 8, 1, _lib.MI_HOST) == _lib.MI_ERR_INVALID
    assert lib.mi_ivfpq_add(fake, P(q), 2, 7, 8, 1, _lib.MI_HOST) == _lib.MI_ERR_INVALID and b"dtype" in lib.mi_last_error()
    assert lib.mi_ivfpq_info(None, None, None, None, None, None, None, None, None, None) == _lib.MI_ERR_INVALID
    assert lib.mi_ivfpq_list_sizes(None, P(idx)) == _lib.MI_ERR_INVALID
    assert lib.mi_ivfpq_list_sizes(fake, None) == _lib.MI_ERR_INVALID
    assert lib.mi_ivfpq_get_rows(None, 0, 1, P(codes), P(lists)) == _lib.MI_ERR_INVALID


def _seeded(seed, n=400, M=4, Ks=16, L=3, nlist=6, nq=9):
    rng = np.random.default_rng(seed)
    C_ = rng.standard_normal((M, Ks, L)).astype(np.float32)
    G = rng.standard_normal((nlist, M * L)).astype(np.float32)
    codes = rng.integers(0, Ks, size=(n, M), dtype=np.uint8)
    lists = rng.integers(0, nlist, size=n).astype(np.uint8)
    q = rng.standard_normal((nq, M * L)).astype(np.float32)
    return C_, G, codes, lists, q


def test_probe_truth_on_a_hand_example():
    G = np.array([[0.0, 0.0], [3.0, 0.0], [0.0, 0.0], [1.0, 1.0]], np.float32)          # lists 0 and 2 coincide
    x = np.array([[0.1, 0.0], [2.9, 0.1], [1.0, 1.0]])
    assert np.array_equal(probe_truth(x, G, 4), [[0, 2, 3, 1], [1, 3, 0, 2], [3, 0, 2, 1]])
    assert np.array_equal(probe_truth(x, G, 1), [[0], [1], [3]])
    assert probe_truth(x, G, 2).dtype == np.int32


def test_truth_with_every_list_probed_is_pq_truth():
    C_, G, codes, lists, q = _seeded(3)
    codes[77], codes[301] = codes[5], codes[5]                            # exact ties across and inside lists
    lists[5], lists[77], lists[301] = 0, 0, 4
    every = np.tile(np.arange(6), (q.shape[0], 1))
    allowed = np.random.default_rng(4).random(400) < 0.6
    for k in (1, 50, 450):
        for al in (None, allowed):
            got = ivfpq_truth(q, C_, codes, lists, every, k, row_offset=1000, allowed=al)
            want = pq_truth(q, C_, codes, k, row_offset=1000, allowed=al)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    assert np.array_equal(ivfpq_truth(q, C_, codes, lists, probe_truth(q, G, 6), 50)[0], pq_truth(q, C_, codes, 50)[0])
    # -1 and repeats do not change the set; no list at all is an all-padding answer
    messy = np.concatenate([every[:, ::-1], every[:, :2], np.full((q.shape[0], 1), -1)], axis=1)
    assert np.array_equal(ivfpq_truth(q, C_, codes, lists, messy, 50)[0], pq_truth(q, C_, codes, 50)[0])
    ids, dist = ivfpq_truth(q, C_, codes, lists, np.full((q.shape[0], 2), -1), 3)
    assert (ids == -1).all() and np.isposinf(dist).all()


def test_truth_with_one_bucket_is_what_the_reference_computes():
    """matching_PQ_Net_bucket (src/utils/nnsearch.py:988-995) given labels and buckets, restated in numpy: the rows of the query's
    bucket, the sums of their table entries, an argsort, and the map back through the bucket's row numbers.  The table here is
    the contract's (float64 sums rounded once) and the sums run in book order, so that on a problem without distance ties the
    two orders are the same and == applies."""
    C_, G, codes, lists, q = _seeded(11, Ks=200)               # 200^4 code rows: the 400 drawn are distinct
    M, K = C_.shape[0], 7
    bucket = probe_truth(q, G, 1)[:, 0]
    T32 = dtable64(q, C_)[1]                                              # [Q, M, Ks]
    want = np.zeros((q.shape[0], K), np.int64)
    for i in range(q.shape[0]):
        bucketind = np.where(bucket[i] == lists)
        refined = codes[bucketind[0], :].astype(np.int64)
        d = np.zeros(refined.shape[0], np.float32)
        for m in range(M):
            d = d + T32[i, m, refined[:, m]]
        assert refined.shape[0] >= K and np.unique(d).size == d.size       # the seeded problem has no ties and no short bucket
        want[i] = bucketind[0][np.argsort(d)[:K]]
    got, _ = ivfpq_truth(q, C_, codes, lists, bucket[:, None], K)
    assert np.array_equal(got, want)
    assert all(np.isin(got[i], np.flatnonzero(lists == bucket[i])).all() for i in range(q.shape[0]))


def test_wrapper_and_index_reject_bad_input_before_the_device(built_lib):
    _, _lib = built_lib
    from isehr_amd.nnsearch import matching_PQ_Net_bucket_hip
    rng = np.random.default_rng(1)
    cw = rng.standard_normal((16, 8)).astype(np.float32)
    q = rng.standard_normal((3, 8)).astype(np.float32)
    codes = rng.integers(0, 16, size=(40, 4))
    gal = rng.standard_normal((40, 8)).astype(np.float32)
    with pytest.raises(ValueError, match="multiple of N_books"):
        matching_PQ_Net_bucket_hip(2, cw, q, 3, codes[:, :3], gal)
    with pytest.raises(ValueError, match="N_words = 257"):
        matching_PQ_Net_bucket_hip(2, np.zeros((257, 8), np.float32), q, 4, codes, gal)
    with pytest.raises(ValueError, match=r"\[0, Ks = 16\)"):
        matching_PQ_Net_bucket_hip(2, cw, q, 4, codes + 12, gal)
    with pytest.raises(ValueError, match="integer array"):
        matching_PQ_Net_bucket_hip(2, cw, q, 4, codes.astype(np.float32), gal)
    with pytest.raises(ValueError, match="K = 0"):
        matching_PQ_Net_bucket_hip(0, cw, q, 4, codes, gal)
    with pytest.raises(ValueError, match="K = 41"):
        matching_PQ_Net_bucket_hip(41, cw, q, 4, codes, gal)
    with pytest.raises(ValueError, match="Gallery_features has 39 rows"):
        matching_PQ_Net_bucket_hip(2, cw, q, 4, codes, gal[:39])
    with pytest.raises(ValueError, match="expected Codewords"):
        matching_PQ_Net_bucket_hip(2, cw, q, 4, codes, gal[:, :4])
    with pytest.raises(ValueError, match="n_clusters = 1"):
        matching_PQ_Net_bucket_hip(2, cw, q, 4, codes, gal, n_clusters=1)
    with pytest.raises(ValueError, match="n_clusters = 257"):
        matching_PQ_Net_bucket_hip(2, cw, q, 4, codes, gal, n_clusters=257)
    with pytest.raises(ValueError, match="nprobe = 0"):
        matching_PQ_Net_bucket_hip(2, cw, q, 4, codes, gal, nprobe=0)
    with pytest.raises(ValueError, match="nprobe = 11"):
        matching_PQ_Net_bucket_hip(2, cw, q, 4, codes, gal, nprobe=11)
    with pytest.raises(ValueError, match="Query must be a finite"):
        matching_PQ_Net_bucket_hip(2, cw, np.full((3, 8), np.nan, np.float32), 4, codes, gal)
    with pytest.raises(ValueError, match="Gallery_features must be a finite"):
        matching_PQ_Net_bucket_hip(2, cw, q, 4, codes, np.where(np.arange(8) == 1, np.inf, gal))
    with pytest.raises(ValueError, match="training rows"):
        matching_PQ_Net_bucket_hip(2, cw, q, 4, codes, gal, n_clusters=41)
    books = np.ascontiguousarray(cw.reshape(16, 4, 2).transpose(1, 0, 2))
    G = rng.standard_normal((5, 8)).astype(np.float32)
    lists = rng.integers(0, 5, size=40)
    IV = _lib.IVFPQIndex
    with pytest.raises(ValueError, match="nlist = 1 "):
        IV.from_codes(G[:1], books, codes, lists * 0)
    with pytest.raises(ValueError, match="nlist = 257"):
        IV.from_codes(np.zeros((257, 8), np.float32), books, codes, lists)
    with pytest.raises(ValueError, match="coarse centroids of 4 columns"):
        IV.from_codes(G[:, :4], books, codes, lists)
    with pytest.raises(ValueError, match="coarse centroids must be finite"):
        IV.from_codes(np.where(np.arange(8) == 1, np.nan, G), books, codes, lists)
    with pytest.raises(ValueError, match="codebooks must be finite"):
        IV.from_codes(G, np.where(np.arange(2) == 1, np.nan, books), codes, lists)
    with pytest.raises(ValueError, match=r"\[0, nlist = 5\)"):
        IV.from_codes(G, books, codes, lists + 1)
    with pytest.raises(ValueError, match=r"\[0, nlist = 5\)"):
        IV.from_codes(G, books, codes, lists - 1)
    with pytest.raises(ValueError, match="list ids must be an integer"):
        IV.from_codes(G, books, codes, lists.astype(np.float32))
    with pytest.raises(ValueError, match=r"list ids must be \[rows = 40\]"):
        IV.from_codes(G, books, codes, lists[:39])
    with pytest.raises(ValueError, match=r"\[0, Ks = 16\)"):
        IV.from_codes(G, books, codes + 12, lists)
    with pytest.raises(ValueError, match="capacity"):
        IV.from_codes(G, books, codes, lists, capacity=3)
    with pytest.raises(ValueError, match="capacity"):
        IV.empty(G, books, 0)
    with pytest.raises(ValueError, match="nlist = 300"):
        IV.fit(gal, 300, 4, 16)
    # the checks of a live index's methods, on an object that has the attributes but no handle
    idx = IV.__new__(IV)
    idx._h, idx.n, idx.d, idx.m, idx.ks, idx.nlist, idx.row_offset = None, 40, 8, 4, 16, 5, 0
    for bad in (0, 6):
        with pytest.raises(ValueError, match="nprobe = %d" % bad):
            idx.search(q, 2, nprobe=bad)
        with pytest.raises(ValueError, match="nprobe = %d" % bad):
            idx.probe(q, bad)
    for bad in (5, -2):
        with pytest.raises(ValueError, match=r"probes must be -1 or lie in \[0, nlist = 5\)"):
            idx.search(q, 2, probes=np.array([[0, 1], [bad, 2], [3, 4]]))
    with pytest.raises(ValueError, match="probes must be an integer array"):
        idx.search(q, 2, probes=np.zeros((2, 2), np.int32))
    with pytest.raises(ValueError, match="rows of 4 columns"):
        idx.search(q[:, :4], 2)
    with pytest.raises(ValueError, match="at most one of allow"):
        idx.search(q, 2, allow=np.ones(40, bool), allow_ptr=64)
    with pytest.raises(ValueError, match=r"\[0, nlist = 5\)"):
        idx.append_codes(codes, lists + 1)
