"""CPU: the PQ index (mi_pq_*) is exported and bound, answers bad arguments before touching a device, the numpy truth
(tests/_pq_truth.py) agrees tie-aware with what the reference's matching_PQ_Net returned for the golden inputs, and
matching_PQ_Net_hip / PQIndex reject bad input with ValueError before the device."""
import ctypes as C
import os

import numpy as np
import pytest

from _pq_truth import adc_truth, books_of, dtable64, encode_truth, pq_truth, tie_aware_vs_reference

NEW = {"mi_pq_create": 12, "mi_pq_append_codes": 5, "mi_pq_add": 7, "mi_pq_encode": 8, "mi_pq_dtable": 7, "mi_pq_search": 12,
       "mi_pq_search_device": 8, "mi_pq_info": 9, "mi_pq_get_codes": 4, "mi_pq_get_codebooks": 2, "mi_pq_destroy": 1}
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pq_net.npz")


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
    for meth in ("from_codes", "empty", "append_codes", "add", "encode", "dtable", "search", "search_device", "get_codes", "codebooks",
                 "close", "__enter__", "__exit__"):
        assert hasattr(_lib.PQIndex, meth), meth
    from isehr_amd import nnsearch
    assert callable(nnsearch.matching_PQ_Net_hip)
    assert nnsearch.matching_PQ_Net_hip not in nnsearch.MATCHING_METHODS.values()
    assert lib.mi_pq_destroy(None) == 0


def test_global_option_pq_matrix_bytes(built_lib):
    lib, _lib = built_lib
    assert _lib.get_global_option("pq_matrix_bytes") == 2 << 30
    _lib.set_global_option("pq_matrix_bytes", 4096)
    assert _lib.get_global_option("pq_matrix_bytes") == 4096
    _lib.set_global_option("pq_matrix_bytes", 0)
    assert _lib.get_global_option("pq_matrix_bytes") == 2 << 30
    assert lib.mi_set_global_option(b"pq_matrix_bytes", -1.0) == 1 and b"pq_matrix_bytes" in lib.mi_last_error()


def test_invalid_arguments_answer_without_a_device(built_lib):
    lib, _lib = built_lib
    P = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    cb = np.random.default_rng(0).standard_normal((4, 16, 2)).astype(np.float32)       # m = 4, ks = 16, L = 2, d = 8
    big = np.zeros(65 * 2 * 64 + 257 * 8 + 5000, np.float32)                            # codebooks for the out-of-range shapes
    codes = np.zeros((3, 4), np.uint8)
    h = C.c_void_p()

    def create(cbp=None, d=8, m=4, ks=16, cd=P(codes), n=3, stride=4, cap=0, out=C.byref(h)):
        return lib.mi_pq_create(P(cb) if cbp is None else cbp, d, m, ks, cd, n, stride, _lib.MI_HOST, 0, 0, cap, out)

    cases = [(dict(out=None), b"out"), (dict(m=0, cbp=P(big)), b"m (books)"), (dict(m=65, d=130, cbp=P(big)), b"m (books)"),
             (dict(ks=1, cbp=P(big)), b"ks (codewords"), (dict(ks=257, cbp=P(big)), b"ks (codewords"),
             (dict(d=9, cbp=P(big)), b"multiple of m"), (dict(d=4100, cbp=P(big)), b"d must be in"), (dict(d=0), b"d must be in"),
             (dict(cap=2), b"capacity"), (dict(cap=-1), b"capacity"), (dict(n=-1), b"negative number of rows"),
             (dict(cd=None), b"codes"), (dict(cd=None, n=0), b"capacity"), (dict(stride=3), b"row_stride_bytes")]
    for kwargs, word in cases:
        assert create(**kwargs) == _lib.MI_ERR_INVALID, kwargs
        assert word in lib.mi_last_error(), (kwargs, lib.mi_last_error())
    assert lib.mi_pq_create(None, 8, 4, 16, P(codes), 3, 4, _lib.MI_HOST, 0, 0, 0, C.byref(h)) == _lib.MI_ERR_INVALID
    assert b"codebooks" in lib.mi_last_error()
    for bad_value in (np.nan, np.inf):
        bad_cb = cb.copy()
        bad_cb[3, 15, 1] = bad_value
        assert create(cbp=P(bad_cb)) == _lib.MI_ERR_INVALID
        assert b"finite" in lib.mi_last_error()
    bad_codes = codes.copy()
    bad_codes[2, 3] = 16
    assert create(cd=P(bad_codes)) == _lib.MI_ERR_INVALID
    assert b">= ks" in lib.mi_last_error()
    assert h.value is None

    q = np.zeros((2, 8), np.float32)
    idx = np.zeros(8, np.int64)
    fake = C.c_void_p(16)                         # non-null, never dereferenced: these checks answer before the handle is read

    def search(hh=fake, k=4, nq=2):
        return lib.mi_pq_search(hh, P(q), nq, _lib.MI_F32, 8, 1, k, None, _lib.MI_HOST, P(idx), None, None)

    def search_dev(hh=fake, k=4, nq=2):
        return lib.mi_pq_search_device(hh, P(q), nq, k, None, P(idx), None, None)

    for fn in (search, search_dev):
        for kwargs, word in [(dict(hh=None), b"null handle"), (dict(k=0), b"k must"), (dict(k=2049), b"k must"),
                             (dict(nq=-1), b"nq must")]:
            assert fn(**kwargs) == _lib.MI_ERR_INVALID, (fn.__name__, kwargs)
            assert word in lib.mi_last_error(), (fn.__name__, kwargs, lib.mi_last_error())
    assert lib.mi_pq_append_codes(None, P(codes), 3, 4, _lib.MI_HOST) == _lib.MI_ERR_INVALID
    assert lib.mi_pq_add(None, P(q), 2, _lib.MI_F32, 8, 1, _lib.MI_HOST) == _lib.MI_ERR_INVALID
    assert lib.mi_pq_encode(None, P(q), 2, _lib.MI_F32, 8, 1, _lib.MI_HOST, P(codes)) == _lib.MI_ERR_INVALID
    assert lib.mi_pq_dtable(None, P(q), 2, _lib.MI_F32, 8, 1, P(q)) == _lib.MI_ERR_INVALID
    assert lib.mi_pq_info(None, None, None, None, None, None, None, None, None) == _lib.MI_ERR_INVALID
    assert lib.mi_pq_get_codes(None, 0, 1, P(codes)) == _lib.MI_ERR_INVALID
    assert lib.mi_pq_get_codebooks(None, P(q)) == _lib.MI_ERR_INVALID


def test_truth_helpers_on_a_hand_example():
    # one book of two codewords in one dimension: entries (x - c)^2; two books: sums in book order
    C1 = np.array([[[0.0], [2.0]], [[1.0], [1.0]]], np.float32)             # M = 2, Ks = 2, L = 1
    x = np.array([[0.5, 3.0], [2.0, 1.0]], np.float64)
    acc, T = dtable64(x, C1)
    assert np.array_equal(acc, [[[0.25, 2.25], [4.0, 4.0]], [[4.0, 0.0], [0.0, 0.0]]])
    assert T.dtype == np.float32 and np.array_equal(T, acc.astype(np.float32))
    assert np.array_equal(encode_truth(x, C1), [[0, 0], [1, 0]])             # equal codewords: the lower index
    codes = np.array([[0, 0], [1, 1], [1, 0], [0, 1]])
    assert np.array_equal(adc_truth(T, codes), [[4.25, 6.25, 6.25, 4.25], [4.0, 0.0, 0.0, 4.0]])
    ids, dist = pq_truth(x, C1, codes, 5, row_offset=10)
    assert np.array_equal(ids, [[10, 13, 11, 12, -1], [11, 12, 10, 13, -1]])
    assert np.array_equal(dist[:, :4], [[4.25, 4.25, 6.25, 6.25], [0, 0, 4, 4]]) and np.isinf(dist[:, 4]).all()
    ids, _ = pq_truth(x, C1, codes, 2, allowed=np.array([False, True, False, True]))
    assert np.array_equal(ids, [[3, 1], [1, 3]])
    # an entry beyond float32 is +inf, a float64 query keeps its low bits
    acc, T = dtable64(np.array([[3e20, 1.0 + 2.0 ** -40]]), C1)
    assert np.isinf(T[0, 0]).all() and acc[0, 1, 0] == 2.0 ** -80


def test_pruned_encode_truth_is_the_plain_argmin():
    """encode_truth's candidate pruning returns what np.argmin of the float64 table returns: duplicated codewords, rows that are
    exact codewords, rows halfway between two codewords (tied or nearly tied sums), float32 and float64 rows"""
    for M, Ks, L in [(1, 2, 1), (3, 16, 5), (8, 255, 2), (4, 256, 32)]:
        rng = np.random.default_rng(M * Ks + L)
        C = rng.standard_normal((M, Ks, L)).astype(np.float32)
        C[0, Ks - 1] = C[0, 0]
        x = rng.standard_normal((300, M * L))
        x[:40] = np.concatenate([C[m, (np.arange(40) * 7 + m) % Ks] for m in range(M)], axis=1)
        x[40:80] = np.concatenate([(C[m, (np.arange(40) + m) % Ks].astype(np.float64) + C[m, (np.arange(40) * 3 + 1) % Ks]) / 2
                                   for m in range(M)], axis=1)
        for rows in (x, x.astype(np.float32)):
            plain = encode_truth(rows, C, prune=False)
            assert np.array_equal(plain, np.argmin(dtable64(rows, C)[0], axis=-1))
            assert np.array_equal(encode_truth(rows, C), plain), (M, Ks, L)


def test_golden_truth_agrees_with_the_reference():
    z = np.load(GOLD)
    cw, query, codes, M, K, idx_ref = z["codewords"], z["query"], z["codes"], int(z["n_books"]), int(z["K"]), z["idx"]
    assert cw.shape == (256, 128) and query.shape == (7, 128) and codes.shape == (2000, 16) and codes.dtype == np.uint8
    assert (M, K) == (16, 100) and idx_ref.shape == (7, 100)
    ours, dist = pq_truth(query, books_of(cw, M), codes, K)
    assert tie_aware_vs_reference(idx_ref, ours, cw, query, M, codes) == []
    assert (ours == idx_ref).mean() > 0.9
    # the fixture has what it is for: duplicated code rows, a tied pair among the first K in (distance, id) order
    assert len(np.unique(codes, axis=0)) == 2000 - 20
    tied = [(q, j) for q in range(7) for j in range(K - 1) if dist[q, j] == dist[q, j + 1]]
    assert tied and all(ours[q, j] < ours[q, j + 1] for q, j in tied)
    # and the comparison can fail: one swapped-in far row is a complaint
    worse = ours.copy()
    worse[2, 5] = np.setdiff1d(np.arange(2000), ours[2])[-1]
    assert tie_aware_vs_reference(idx_ref, worse, cw, query, M, codes) != []


def test_wrapper_and_index_reject_bad_input_before_the_device(built_lib):
    _, _lib = built_lib
    from isehr_amd.nnsearch import matching_PQ_Net_hip
    rng = np.random.default_rng(1)
    cw = rng.standard_normal((16, 8)).astype(np.float32)
    q = rng.standard_normal((3, 8)).astype(np.float32)
    codes = rng.integers(0, 16, size=(5, 4))
    with pytest.raises(ValueError, match="multiple of N_books"):
        matching_PQ_Net_hip(2, cw, q, 3, codes[:, :3])
    with pytest.raises(ValueError, match="N_words = 257"):
        matching_PQ_Net_hip(2, np.zeros((257, 8), np.float32), q, 4, codes)
    with pytest.raises(ValueError, match=r"\[0, Ks = 16\)"):
        matching_PQ_Net_hip(2, cw, q, 4, codes + 12)
    with pytest.raises(ValueError, match=r"\[0, Ks = 16\)"):
        matching_PQ_Net_hip(2, cw, q, 4, codes - 16)
    with pytest.raises(ValueError, match="integer array"):
        matching_PQ_Net_hip(2, cw, q, 4, codes.astype(np.float32))
    with pytest.raises(ValueError, match="K = 0"):
        matching_PQ_Net_hip(0, cw, q, 4, codes)
    with pytest.raises(ValueError, match="K = 6"):
        matching_PQ_Net_hip(6, cw, q, 4, codes)
    with pytest.raises(ValueError, match="K <= 2048"):
        matching_PQ_Net_hip(2049, cw, q, 4, rng.integers(0, 16, size=(3000, 4)))
    with pytest.raises(ValueError, match="N_books = 4"):
        matching_PQ_Net_hip(2, cw, q, 4, codes[:, :3])
    with pytest.raises(ValueError, match="expected Codewords"):
        matching_PQ_Net_hip(2, cw, q[:, :4], 4, codes)
    with pytest.raises(ValueError, match="finite"):
        matching_PQ_Net_hip(2, cw, np.full((3, 8), np.nan, np.float32), 4, codes)
    books = books_of(cw, 4)
    with pytest.raises(ValueError, match="Ks = 257"):
        _lib.PQIndex.from_codes(np.zeros((1, 257, 2), np.float32), codes[:, :1])
    with pytest.raises(ValueError, match="M = 65"):
        _lib.PQIndex.from_codes(np.zeros((65, 4, 1), np.float32), np.zeros((5, 65), np.uint8))
    with pytest.raises(ValueError, match="d = M"):
        _lib.PQIndex.from_codes(np.zeros((2, 4, 2049), np.float32), codes[:, :2] % 4)
    with pytest.raises(ValueError, match="finite"):
        _lib.PQIndex.from_codes(np.where(np.arange(2) == 1, np.nan, books), codes)
    with pytest.raises(ValueError, match=r"\[0, Ks = 16\)"):
        _lib.PQIndex.from_codes(books, codes + 12)
    with pytest.raises(ValueError, match="integer array"):
        _lib.PQIndex.from_codes(books, codes.astype(np.float64))
    with pytest.raises(ValueError, match="capacity"):
        _lib.PQIndex.from_codes(books, codes, capacity=3)
    with pytest.raises(ValueError, match="capacity"):
        _lib.PQIndex.empty(books, 0)
