"""CPU: the squared-L2 entry points (mi_gallery_create_l2, mi_knn_search_l2, mi_knn_search_l2_device, mi_knn_dense64_search_l2)
are exported and bound, answer bad arguments before touching a device, and the three-way split of the bias -1/2 ||g||^2
(csrc/l2_metric.hip l2_bias_kernel, restated in numpy) sums back to it in float64 for both 16-bit image types."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _gallery_file import split_bias  # noqa: E402  (the numpy restatement of l2_bias_kernel, shared with test_gallery_reference_cpu.py)

NEW = ["mi_gallery_create_l2", "mi_knn_search_l2", "mi_knn_search_l2_device", "mi_knn_dense64_search_l2"]


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__
    __graft_entry__.build()
    from isehr_amd import _lib
    return _lib.load(), _lib


def test_symbols_are_exported_and_bound(built_lib):
    lib, _lib = built_lib
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name).restype == C.c_int
    assert len(_lib.SIGNATURES["mi_gallery_create_l2"][1]) == 11
    assert len(_lib.SIGNATURES["mi_knn_search_l2"][1]) == 14
    assert (_lib.METRIC_IP, _lib.METRIC_L2) == (0, 1)
    for meth in ("l2_from_host", "l2_from_device_ptr", "search_l2", "dense64_search_l2", "search_l2_device"):
        assert hasattr(_lib.Gallery, meth)


def test_invalid_arguments_answer_without_a_device(built_lib):
    lib, _lib = built_lib
    q = np.zeros((2, 4), np.float32)
    idx = np.zeros(8, np.int64)
    P = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    fake = C.c_void_p(16)                         # non-null, never dereferenced: these checks answer before the handle is read

    def search(g=fake, k=4, nq=2, dtype=_lib.MI_F32):
        return lib.mi_knn_search_l2(g, P(q), nq, dtype, 4, 1, k, None, _lib.MI_HOST, P(idx), None, None, None, None)

    for kwargs, word in [(dict(g=None), b"null"), (dict(k=0), b"k must"), (dict(k=2049), b"k must"), (dict(k=-3), b"k must"),
                         (dict(nq=-1), b"nq"), (dict(dtype=9), b"dtype")]:
        assert search(**kwargs) == _lib.MI_ERR_INVALID, kwargs
        assert word in lib.mi_last_error(), (kwargs, lib.mi_last_error())
    assert lib.mi_knn_search_l2_device(None, P(q), 2, 4, P(idx), None, None, None) == _lib.MI_ERR_INVALID
    assert lib.mi_knn_search_l2_device(fake, P(q), 2, 0, P(idx), None, None, None) == _lib.MI_ERR_INVALID
    assert lib.mi_knn_search_l2_device(fake, P(q), 2, 2049, P(idx), None, None, None) == _lib.MI_ERR_INVALID
    assert b"k must" in lib.mi_last_error()
    assert lib.mi_knn_dense64_search_l2(None, P(q), 2, _lib.MI_F32, 4, 1, 4, P(idx), None, None, None) == _lib.MI_ERR_INVALID
    assert lib.mi_knn_dense64_search_l2(fake, P(q), 2, _lib.MI_F32, 4, 1, 4097, P(idx), None, None, None) == _lib.MI_ERR_INVALID
    assert lib.mi_knn_dense64_search_l2(fake, P(q), 2, _lib.MI_F32, 4, 1, 0, P(idx), None, None, None) == _lib.MI_ERR_INVALID
    h = C.c_void_p()
    for n, d, cap, data, word in [(-1, 4, 0, P(q), b"negative number of rows"), (2, 0, 0, P(q), b"d must"),
                                  (2, 4, -1, P(q), b"capacity"), (2, 4, 0, None, b"data"), (0, 4, 0, None, b"capacity"),
                                  (2, 4, 1, P(q), b"capacity")]:
        rc = lib.mi_gallery_create_l2(data, n, d, _lib.MI_F32, 4, 1, _lib.MI_HOST, 0, 0, cap, C.byref(h))
        assert rc == _lib.MI_ERR_INVALID, (n, d, cap)
        assert word in lib.mi_last_error(), (n, d, cap, lib.mi_last_error())
    assert lib.mi_gallery_create_l2(P(q), 2, 4, _lib.MI_F32, 4, 1, _lib.MI_HOST, 0, 0, 0, None) == _lib.MI_ERR_INVALID


def _bf16(x32):
    """float32 -> nearest-even bfloat16, returned as float32"""
    u = np.asarray(x32, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


@pytest.mark.parametrize("f16", [True, False])
def test_bias_split_sums_back_in_float64(f16):
    rng = np.random.default_rng(5)
    # (1/2 * 362^2 = 65 522 is the first bias beyond fp16's 65 504: the range goes well past it)
    norms = np.concatenate([np.geomspace(1e-3, 3000.0, 500), [1e-3, 1.0, 300.0, 361.0, 362.0, 363.0, 512.0, 3000.0]])
    X = rng.standard_normal((len(norms), 2048)).astype(np.float32)
    X = (X * (norms / np.linalg.norm(X.astype(np.float64), axis=1))[:, None]).astype(np.float32)
    b, c1, c2, c3 = split_bias(X, f16)
    assert np.isfinite(c1).all()
    total = (c1.astype(np.float64) + c2.astype(np.float64)) + c3.astype(np.float64)
    inside = np.abs(b) <= 65504.0 if f16 else np.ones(len(b), bool)
    assert (total[inside] == b[inside]).all(), np.abs(total - b)[inside].max()
    # beyond fp16's range the clamped c1 leaves c2 + c3 (24 + 24 bits) short of b's 53: finite and good to 2^-47, which is all
    # that pass needs -- such a row's augmented norm is far above 4, so the create loop re-ingests the gallery as bf16, where
    # the split is exact again (the bf16 case of this test covers the same norms)
    assert (np.abs(total - b)[~inside] <= np.abs(b[~inside]) * 2.0 ** -47).all()
    # c1 is exact in the image type, and what the 16-bit image loses of c2 / c3 is tiny next to the bias
    back = c1.astype(np.float16).astype(np.float32) if f16 else _bf16(c1)
    assert (back == c1).all()
    assert (np.abs(c2[inside]) <= np.abs(b[inside]) * (2.0 ** -10 if f16 else 2.0 ** -7) + 2.0 ** -24).all()
    if f16:                                        # beyond the range c1 is the clamp and c2 carries the rest
        assert (c1[~inside] == np.float32(-65504.0)).all() and (~inside).sum() > 50


def test_knn_methods(built_lib):
    _, _lib = built_lib
    from isehr_amd.knn import KNN
    with pytest.raises(NotImplementedError):
        KNN(np.zeros((4, 4), np.float32), "manhattan")
    calls = []

    class FakeGallery:
        def search_l2(self, q, k, allow=None):
            calls.append((q.dtype, q.shape, k, allow))
            return (np.zeros((q.shape[0], k), np.int64), np.ones((q.shape[0], k), np.float32), None, {}, 0.0)

    knn = object.__new__(KNN)
    knn.gallery, knn.method, knn.N, knn.D = FakeGallery(), "euclidean", 10, 4
    dist, ids = knn.search(np.zeros((3, 4), np.float64), 2)
    assert dist.dtype == np.float32 and ids.dtype == np.int64 and dist.shape == ids.shape == (3, 2)
    assert calls == [(np.float32, (3, 4), 2, None)]
    with pytest.raises(NotImplementedError):
        knn.range_search(np.zeros((3, 4), np.float32), 0.5)
