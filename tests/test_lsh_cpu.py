"""CPU: the LSH entry points (mi_lsh_encode*, mi_hamming_append_lsh_device) are exported and bound and answer bad arguments
before touching a device, with a text that names the argument; lsh_rotation is what its docstring says; matching_LSH_hip rejects
bad input before the device; LSHIndex.search is plumbed through to the encoder and the binary gallery."""
import ctypes as C

import numpy as np
import pytest

NEW = {"mi_lsh_encode_device": 12, "mi_lsh_encode": 11, "mi_hamming_append_lsh_device": 10}


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
    for meth in ("from_host", "empty", "add", "add_device", "encode", "search", "get_codes", "close", "__enter__", "__exit__"):
        assert hasattr(_lib.LSHIndex, meth), meth
    assert hasattr(_lib.LSHIndex, "hbm_bytes") and hasattr(_lib.BinaryGallery, "append_lsh_device")
    assert callable(_lib.lsh_rotation) and callable(_lib.lsh_encode) and callable(_lib.lsh_encode_device)


def test_invalid_arguments_answer_without_a_device(built_lib):
    lib, _lib = built_lib
    x = np.zeros((2, 16), np.float32)
    R = np.zeros((8, 16), np.float64)
    out = np.zeros((2, 8), np.uint8)
    P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
    F32, F64 = _lib.MI_F32, _lib.MI_F64

    def dev(X=x, n=2, d=16, dtype=F32, rs=16, cs=1, r=R, nbits=8, o=out, ors=1):
        return lib.mi_lsh_encode_device(P(X), n, d, dtype, rs, cs, P(r), None, nbits, P(o), ors, None)

    def host(X=x, n=2, d=16, dtype=F32, rs=16, cs=1, r=R, nbits=8, o=out, ors=None):
        return lib.mi_lsh_encode(P(X), n, d, dtype, rs, cs, P(r), None, nbits, 0, P(o))

    cases = [(dict(nbits=0), b"nbits"), (dict(nbits=12), b"nbits"), (dict(nbits=4104), b"nbits"), (dict(nbits=-8), b"nbits"),
             (dict(d=0), b"d must"), (dict(d=4097), b"d must"), (dict(n=-1), b"rows: n"), (dict(dtype=2), b"dtype"),
             (dict(dtype=-1), b"dtype"), (dict(X=None), b"X"), (dict(r=None), b"R"), (dict(o=None), b"out"),
             (dict(rs=-1), b"row_stride"), (dict(cs=-1), b"col_stride")]
    for fn in (dev, host):
        for kwargs, word in cases:
            assert fn(**kwargs) == _lib.MI_ERR_INVALID, (fn.__name__, kwargs)
            assert word in lib.mi_last_error(), (fn.__name__, kwargs, lib.mi_last_error())
        # no rows: nothing to do, and no pointer to the rows is needed
        assert fn(n=0) == 0 and fn(n=0, X=None, o=None) == 0
        for dtype in (F32, F64):
            assert fn(n=0, dtype=dtype, nbits=4096, d=4096, ors=512) == 0
    assert dev(ors=0) == _lib.MI_ERR_INVALID and b"out_row_stride_bytes" in lib.mi_last_error()
    assert dev(nbits=16, ors=1) == _lib.MI_ERR_INVALID and b"out_row_stride_bytes" in lib.mi_last_error()
    # the append checks its handle first, then the same operands (nbits is the handle's)
    assert lib.mi_hamming_append_lsh_device(None, P(x), 2, 16, F32, 16, 1, P(R), None, None) == _lib.MI_ERR_INVALID
    assert b"null handle" in lib.mi_last_error()


def test_lsh_rotation(built_lib):
    _, _lib = built_lib
    for d, nbits in [(64, 64), (100, 32), (128, 8)]:
        R = _lib.lsh_rotation(d, nbits)
        assert R.shape == (nbits, d) and R.dtype == np.float64 and R.flags.c_contiguous
        assert np.array_equal(R, _lib.lsh_rotation(d, nbits, seed=5))           # the default seed is faiss's 5; same bits
        assert np.abs(R @ R.T - np.eye(nbits)).max() <= 1e-12
        assert not np.array_equal(R, _lib.lsh_rotation(d, nbits, seed=6))
    # the recipe itself
    q, _ = np.linalg.qr(np.random.RandomState(5).standard_normal((100, 100)))
    assert np.array_equal(_lib.lsh_rotation(100, 32), q[:32, :100])
    # more bits than columns: accepted, the first d columns of a rotation of nbits dimensions (rows no longer orthonormal)
    R = _lib.lsh_rotation(17, 136)
    assert R.shape == (136, 17) and R.dtype == np.float64
    assert np.abs(R.T @ R - np.eye(17)).max() <= 1e-12
    for d, nbits in [(16, 12), (16, 0), (16, 4104), (0, 8), (4097, 8)]:
        with pytest.raises(ValueError):
            _lib.lsh_rotation(d, nbits)


def test_matching_lsh_rejects_bad_input_before_the_device(built_lib):
    from isehr_amd import nnsearch
    from isehr_amd.nnsearch import matching_LSH_hip
    a = np.zeros((5, 16), np.float32)
    for n_bits in (12, 0, 4104, -8):
        with pytest.raises(ValueError, match="n_bits"):
            matching_LSH_hip(2, a, a[:1], n_bits)
    with pytest.raises(ValueError, match="expected rows"):
        matching_LSH_hip(2, a, a[:1, :8], 8)
    with pytest.raises(ValueError, match="expected rows"):
        matching_LSH_hip(2, a, a[0], 8)
    with pytest.raises(ValueError, match="K = 0"):
        matching_LSH_hip(0, a, a[:1], 8)
    with pytest.raises(ValueError, match="K = 6"):
        matching_LSH_hip(6, a, a[:1], 8)
    with pytest.raises(ValueError, match="K <= 2048"):
        matching_LSH_hip(2049, np.zeros((2050, 4), np.float32), a[:1, :4], 8)
    with pytest.raises(ValueError, match="floating"):
        matching_LSH_hip(2, a.astype(np.int64), a[:1], 8)
    with pytest.raises(ValueError, match="d = 4097"):
        matching_LSH_hip(1, np.zeros((1, 4097), np.float32), np.zeros((1, 4097), np.float32), 8)
    assert matching_LSH_hip not in nnsearch.MATCHING_METHODS.values()


def test_lsh_index_search_plumbing(built_lib, monkeypatch):
    """LSHIndex.search on a fake gallery and a recording encoder: what is passed on, and what comes back."""
    import torch
    _, _lib = built_lib
    calls = []

    class FakeBinary:
        n, row_offset, nbits, device = 130, 1000, 16, 0

        def search_device(self, q_ptr, nq, k, idx_ptr, dist_ptr=None, allow_ptr=None, stream=None):
            calls.append(("search", q_ptr, nq, k, idx_ptr != 0, dist_ptr is not None, allow_ptr, stream))

    def fake_encode(x_ptr, n, d, r_ptr, nbits, out_ptr, thr_ptr=None, dtype=_lib.MI_F32, row_stride=None, col_stride=1,
                    out_row_stride=None, stream=None):
        calls.append(("encode", n, d, r_ptr, nbits, out_ptr, thr_ptr, dtype, stream))

    monkeypatch.setattr(_lib, "lsh_encode_device", fake_encode)
    idx = object.__new__(_lib.LSHIndex)
    idx.gallery, idx.nbits, idx.d, idx._tdev = FakeBinary(), 16, 4, "cpu"
    idx._R, idx._thr = torch.zeros((16, 4), dtype=torch.float64), None
    idx._stream = lambda: 77
    ids, dist, secs = idx.search(np.zeros((3, 4), np.float64), 2)
    assert ids.dtype == np.int64 and dist.dtype == np.int32 and ids.shape == dist.shape == (3, 2) and secs >= 0.0
    (e, n, d, r_ptr, nbits, out_ptr, thr_ptr, dtype, s1), (s, q_ptr, nq, k, has_idx, has_dist, allow_ptr, s2) = calls
    assert (e, n, d, nbits, thr_ptr, dtype, s1) == ("encode", 3, 4, 16, None, _lib.MI_F64, 77)
    assert r_ptr == idx._R.data_ptr()
    assert (s, nq, k, has_idx, has_dist, allow_ptr, s2) == ("search", 3, 2, True, True, None, 77)
    assert q_ptr == out_ptr                                  # the search reads the codes the encoder wrote
    # thresholds and an allow list of global ids reach the device calls as pointers
    del calls[:]
    idx._thr = torch.zeros(16, dtype=torch.float64)
    idx.search(np.zeros((1, 4), np.float32), 5, allow=[1000, 1129])
    assert calls[0][6] == idx._thr.data_ptr() and calls[0][7] == _lib.MI_F32 and calls[1][6] not in (None, 0)
    # bad input is answered before anything is enqueued
    del calls[:]
    with pytest.raises(ValueError, match="columns"):
        idx.search(np.zeros((3, 5), np.float32), 2)
    with pytest.raises(ValueError, match="k must"):
        idx.search(np.zeros((3, 4), np.float32), 0)
    with pytest.raises(ValueError, match="k must"):
        idx.search(np.zeros((3, 4), np.float32), 2049)
    with pytest.raises(ValueError):
        idx.search(np.zeros((3, 4), np.float32), 2, allow=[999])
    assert calls == []
    ids, dist, _ = idx.search(np.zeros((0, 4), np.float32), 2)
    assert ids.shape == dist.shape == (0, 2) and calls == []
    idx.gallery = None                                       # nothing to close
