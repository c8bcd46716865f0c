"""CPU: the binary index (mi_hamming_*, mi_pack_sign_bits_device) is exported and bound, answers bad arguments before touching a
device, pack_bits follows np.packbits(bitorder='little'), the stable numpy restatement of matching_Greedyhash agrees (tie-aware)
with what the reference returned for the golden inputs, and KNN(..., 'hamming') is plumbed through."""
import ctypes as C
import os

import numpy as np
import pytest

from _hamming_truth import greedyhash_restated, hamming_truth, tie_aware_equal

NEW = {"mi_hamming_create": 9, "mi_hamming_append": 5, "mi_hamming_append_sign_device": 6, "mi_pack_sign_bits_device": 7,
       "mi_hamming_info": 7, "mi_hamming_get_codes": 4, "mi_hamming_search": 10, "mi_hamming_search_device": 8,
       "mi_hamming_destroy": 1}
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "greedyhash.npz")


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
    for meth in ("from_host", "empty", "append", "append_sign_device", "search", "search_device", "get_codes", "close"):
        assert hasattr(_lib.BinaryGallery, meth), meth
    assert callable(_lib.pack_bits) and callable(_lib.pack_sign_bits_device)
    from isehr_amd import nnsearch
    assert callable(nnsearch.matching_Greedyhash_hip)
    assert nnsearch.MATCHING_METHODS["Greedyhash"] is nnsearch.matching_Greedyhash_hip
    assert lib.mi_hamming_destroy(None) == 0
    assert _lib.get_global_option("hamming_matrix_bytes") == 2 << 30
    _lib.set_global_option("hamming_matrix_bytes", 4096)
    assert _lib.get_global_option("hamming_matrix_bytes") == 4096
    _lib.set_global_option("hamming_matrix_bytes", 0)
    assert _lib.get_global_option("hamming_matrix_bytes") == 2 << 30
    assert lib.mi_set_global_option(b"hamming_matrix_bytes", -1.0) == 1 and b"hamming_matrix_bytes" in lib.mi_last_error()


def test_invalid_arguments_answer_without_a_device(built_lib):
    lib, _lib = built_lib
    q = np.zeros((2, 8), np.uint8)
    idx = np.zeros(8, np.int64)
    P = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    fake = C.c_void_p(16)                         # non-null, never dereferenced: these checks answer before the handle is read

    def search(h=fake, k=4, nq=2):
        return lib.mi_hamming_search(h, P(q), nq, 8, k, None, _lib.MI_HOST, P(idx), None, None)

    def search_dev(h=fake, k=4, nq=2):
        return lib.mi_hamming_search_device(h, P(q), nq, k, None, P(idx), None, None)

    for fn in (search, search_dev):
        for kwargs, word in [(dict(h=None), b"null handle"), (dict(k=0), b"k must"), (dict(k=2049), b"k must"),
                             (dict(nq=-1), b"nq must")]:
            assert fn(**kwargs) == _lib.MI_ERR_INVALID, (fn.__name__, kwargs)
            assert word in lib.mi_last_error(), (fn.__name__, kwargs, lib.mi_last_error())
    h = C.c_void_p()
    for n, nbits, cap, data, word in [(2, 0, 0, P(q), b"nbits"), (2, 12, 0, P(q), b"nbits"), (2, 4104, 0, P(q), b"nbits"),
                                      (-1, 64, 0, P(q), b"negative number of rows"), (2, 64, 1, P(q), b"capacity"),
                                      (2, 64, -1, P(q), b"capacity"), (2, 64, 0, None, b"codes"), (0, 64, 0, None, b"capacity")]:
        rc = lib.mi_hamming_create(data, n, nbits, 8, _lib.MI_HOST, 0, 0, cap, C.byref(h))
        assert rc == _lib.MI_ERR_INVALID, (n, nbits, cap)
        assert word in lib.mi_last_error(), (n, nbits, cap, lib.mi_last_error())
    assert lib.mi_hamming_create(P(q), 2, 64, 8, _lib.MI_HOST, 0, 0, 0, None) == _lib.MI_ERR_INVALID
    assert b"out" in lib.mi_last_error()
    assert lib.mi_hamming_create(P(q), 2, 64, 4, _lib.MI_HOST, 0, 0, 0, C.byref(h)) == _lib.MI_ERR_INVALID
    assert b"row_stride_bytes" in lib.mi_last_error()
    assert lib.mi_hamming_append(None, P(q), 2, 8, _lib.MI_HOST) == _lib.MI_ERR_INVALID
    assert lib.mi_hamming_append_sign_device(None, P(q), 2, 64, 64, None) == _lib.MI_ERR_INVALID
    assert lib.mi_hamming_info(None, None, None, None, None, None, None) == _lib.MI_ERR_INVALID
    assert lib.mi_hamming_get_codes(None, 0, 1, P(q)) == _lib.MI_ERR_INVALID
    assert lib.mi_pack_sign_bits_device(P(q), 2, 12, 12, P(q), 2, None) == _lib.MI_ERR_INVALID
    assert b"multiple of 8" in lib.mi_last_error()
    assert lib.mi_pack_sign_bits_device(P(q), -1, 16, 16, P(q), 2, None) == _lib.MI_ERR_INVALID
    assert lib.mi_pack_sign_bits_device(None, 2, 16, 16, P(q), 2, None) == _lib.MI_ERR_INVALID


@pytest.mark.parametrize("code_len", [5, 8, 100])
def test_pack_bits(built_lib, code_len):
    _, _lib = built_lib
    rng = np.random.default_rng(code_len)
    for dtype in (np.bool_, np.uint8, np.int32, np.int64):
        a = rng.integers(0, 2, size=(13, code_len)).astype(dtype)
        p = _lib.pack_bits(a)
        assert p.dtype == np.uint8 and p.shape == (13, (code_len + 7) // 8)
        assert np.array_equal(p, np.packbits(a.astype(bool), axis=1, bitorder="little"))
        # bit j of a code is bit j & 7 of byte j >> 3; the padding bits are zero
        for j in (0, code_len // 2, code_len - 1):
            assert np.array_equal((p[:, j >> 3] >> (j & 7)) & 1, a[:, j].astype(np.uint8))
        padded = np.zeros((13, p.shape[1] * 8), np.uint8)
        padded[:, :code_len] = a
        assert np.array_equal(_lib.unpack_bits(p), padded)
        assert np.array_equal(_lib.unpack_bits(p, code_len), a.astype(np.uint8))
    bad = np.zeros((3, code_len), np.int64)
    bad[1, code_len - 1] = 2
    with pytest.raises(ValueError, match="0 and 1"):
        _lib.pack_bits(bad)
    bad[1, code_len - 1] = -1
    with pytest.raises(ValueError, match="0 and 1"):
        _lib.pack_bits(bad)


def test_golden_restatement_agrees_with_the_reference():
    z = np.load(GOLD)
    train, test, K, idx_ref = z["train"], z["test"], int(z["K"]), z["idx"]
    assert train.shape == (400, 64) and test.shape == (7, 64) and K == 10 and idx_ref.shape == (7, 10)
    assert set(np.unique(train)) <= {0, 1} and set(np.unique(test)) <= {0, 1}
    ours = greedyhash_restated(K, train, test)
    assert tie_aware_equal(idx_ref, ours, train, test) == []
    # the fixture has what it is for: copied queries at distance 0 and ties among the first K
    d0 = (test[0].astype(np.int64) ^ train.astype(np.int64)).sum(1)
    assert (d0 == 0).sum() >= 2 and ours[0, 0] == np.flatnonzero(d0 == 0)[0]
    # the packed truth helper is the same function
    packed_ids, _, _ = hamming_truth(np.packbits(train, axis=1, bitorder="little"),
                                     np.packbits(test, axis=1, bitorder="little"), K)
    assert np.array_equal(packed_ids, ours)


def test_greedyhash_rejects_bad_input_before_the_device(built_lib):
    from isehr_amd.nnsearch import matching_Greedyhash_hip
    a = np.zeros((5, 16), np.int64)
    with pytest.raises(ValueError, match="0 and 1"):
        matching_Greedyhash_hip(2, a + 2, a[:1])
    with pytest.raises(ValueError, match="K = 6"):
        matching_Greedyhash_hip(6, a, a[:1])
    with pytest.raises(ValueError, match="integer or bool"):
        matching_Greedyhash_hip(2, a.astype(np.float32), a[:1])
    with pytest.raises(ValueError, match="code_len"):
        matching_Greedyhash_hip(2, a, a[:1, :8])


def test_knn_hamming_plumbing(built_lib):
    from isehr_amd.knn import KNN
    with pytest.raises(NotImplementedError):
        KNN(np.zeros((4, 4), np.float32), "manhattan")
    with pytest.raises(ValueError, match="uint8"):
        KNN(np.zeros((4, 4), np.float32), "hamming")
    calls = []

    class FakeBinary:
        def search(self, q, k, allow=None):
            calls.append((q.dtype, q.shape, k, allow))
            return np.zeros((q.shape[0], k), np.int64), np.ones((q.shape[0], k), np.int32), 0.0

    knn = object.__new__(KNN)
    knn.gallery, knn.method, knn.N, knn.D = FakeBinary(), "hamming", 10, 32
    dist, ids = knn.search(np.zeros((3, 4), np.uint8), 2)
    assert dist.dtype == np.int32 and ids.dtype == np.int64 and dist.shape == ids.shape == (3, 2)
    assert calls == [(np.uint8, (3, 4), 2, None)]
    with pytest.raises(NotImplementedError):
        knn.range_search(np.zeros((3, 4), np.uint8), 3)
    with pytest.raises(NotImplementedError):
        knn.remove_ids([1])
