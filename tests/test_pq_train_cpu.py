"""CPU: learning PQ codebooks (mi_pq_train).  The numpy truth (tests/_pq_train_truth.py) is scipy's kmeans2(minit="matrix") bit
for bit, the symbol is exported and bound, and every refusal of _lib.pq_train / matching_Nano_PQ_hip is a ValueError before the
library is loaded."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from _pq_truth import books_of
from _pq_train_truth import clustered, rows_init, train_truth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (n, M, Ks, L, iters), drawn in this order from ONE RandomState(5)
SCIPY_CASES = [(300, 2, 4, 8, 6), (1000, 3, 16, 5, 8), (2500, 4, 256, 4, 4)]


def test_truth_is_scipy_kmeans2_bit_for_bit():
    vq = pytest.importorskip("scipy.cluster.vq")
    rng = np.random.RandomState(5)
    for case, (n, M, Ks, L, iters) in enumerate(SCIPY_CASES):
        x, init = clustered(rng, n, M, Ks, L)
        C, moved = train_truth(x, M, Ks, iters, rows_init(x, M, init))
        for j in range(M):
            xj = x[:, j * L:(j + 1) * L].astype(np.float64)
            cent, _ = vq.kmeans2(xj, xj[init[j]], iter=iters, minit="matrix")
            assert np.array_equal(cent.astype(np.float32).view(np.uint32), C[j].view(np.uint32)), (case, j)
        if case == 0:
            assert moved.tolist() == [600, 105, 8, 4, 0, 0]         # the early stop and the zero fill


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__
    __graft_entry__.build()
    from isehr_amd import _lib
    return _lib.load(), _lib


def test_symbol_is_declared_exported_and_bound(built_lib):
    lib, _lib = built_lib
    hdr = open(os.path.join(ROOT, "include", "mi355_retrieval.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+mi_pq_train\s*\(", code)
    assert "Out of scope: learning codebooks" not in hdr
    for name, nargs in (("mi_pq_train", 15), ("mi_pq_train_timing", 5)):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
        assert getattr(lib, name).restype == C.c_int and len(_lib.SIGNATURES[name][1]) == nargs, name
    for fn in ("pq_train", "pq_train_device"):
        assert callable(getattr(_lib, fn))
    assert callable(_lib.PQIndex.fit)


def test_c_entry_point_answers_bad_arguments_without_a_device(built_lib):
    lib, _lib = built_lib
    P = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    x = np.random.default_rng(0).standard_normal((20, 8)).astype(np.float32)
    out = np.zeros((4, 16, 2), np.float32)
    init = np.zeros((4, 16, 2), np.float32)

    def train(xp=P(x), n=20, d=8, dtype=_lib.MI_F32, rs=8, cs=1, memspace=_lib.MI_HOST, m=4, ks=16, iters=3, ip=None, op=P(out)):
        return lib.mi_pq_train(xp, n, d, dtype, rs, cs, memspace, m, ks, iters, ip, 0, op, None, None)

    bad_init = init.copy()
    bad_init[3, 15, 1] = np.inf
    bad_rows = x.copy()
    bad_rows[19, 7] = np.nan
    cases = [(dict(xp=None), b"rows"), (dict(op=None), b"out_codebooks_host"), (dict(dtype=2), b"dtype"), (dict(rs=-1), b"strides"),
             (dict(memspace=2), b"memspace"), (dict(m=0), b"m (books)"), (dict(m=65, d=130), b"m (books)"), (dict(ks=1), b"ks (codewords"),
             (dict(ks=257), b"ks (codewords"), (dict(d=0), b"d must be in"), (dict(d=4100), b"d must be in"), (dict(m=3), b"multiple of m"),
             (dict(n=15), b"n >= ks"), (dict(iters=0), b"iters"), (dict(ip=P(bad_init)), b"finite"), (dict(xp=P(bad_rows)), b"finite")]
    for kwargs, word in cases:
        assert train(**kwargs) == _lib.MI_ERR_INVALID, kwargs
        assert word in lib.mi_last_error(), (kwargs, lib.mi_last_error())


def _refuses(monkeypatch):
    from isehr_amd import _lib

    def no_device():
        raise AssertionError("the library was loaded: the refusal came too late")
    monkeypatch.setattr(_lib, "load", no_device)
    return _lib


def test_pq_train_refuses_before_the_device(monkeypatch):
    _lib = _refuses(monkeypatch)
    x = np.random.default_rng(1).standard_normal((40, 8)).astype(np.float32)
    with pytest.raises(ValueError, match="no multiple of M"):
        _lib.pq_train(x, 3, 4)
    with pytest.raises(ValueError, match="Ks = 257"):
        _lib.pq_train(np.zeros((300, 8), np.float32), 4, 257)
    with pytest.raises(ValueError, match="Ks = 1 "):
        _lib.pq_train(x, 4, 1)
    with pytest.raises(ValueError, match="M = 0"):
        _lib.pq_train(x, 0, 4)
    with pytest.raises(ValueError, match="n = 40"):
        _lib.pq_train(x, 4, 64)
    with pytest.raises(ValueError, match="iters = 0"):
        _lib.pq_train(x, 4, 4, iters=0)
    for bad in (np.nan, np.inf):
        y = x.copy()
        y[39, 7] = bad
        with pytest.raises(ValueError, match="finite"):
            _lib.pq_train(y, 4, 4)
    init = np.zeros((4, 4, 2), np.float32)
    rows = np.zeros((4, 4), np.int64)
    for kwargs in (dict(init=init, seed=1), dict(init=init, init_rows=rows), dict(init_rows=rows, seed=1)):
        with pytest.raises(ValueError, match="at most one"):
            _lib.pq_train(x, 4, 4, **kwargs)
    with pytest.raises(ValueError, match=r"\[M, Ks, L\]"):
        _lib.pq_train(x, 4, 4, init=np.zeros((4, 4, 3), np.float32))
    with pytest.raises(ValueError, match="finite"):
        _lib.pq_train(x, 4, 4, init=np.full((4, 4, 2), np.nan, np.float32))
    with pytest.raises(ValueError, match="init_rows"):
        _lib.pq_train(x, 4, 4, init_rows=rows + 40)
    with pytest.raises(ValueError, match="init_rows"):
        _lib.pq_train(x, 4, 4, init_rows=rows[:3])
    with pytest.raises(ValueError, match="n = 3"):
        _lib.pq_train_device(4096, 3, 8, 4, 4, 2)
    with pytest.raises(ValueError, match="no multiple of M"):
        _lib.PQIndex.fit(x, 3, 4)


def test_matching_nano_pq_refuses_before_the_device(monkeypatch):
    _refuses(monkeypatch)
    from isehr_amd import nnsearch
    from isehr_amd.nnsearch import matching_Nano_PQ_hip
    assert nnsearch.MATCHING_METHODS["PQ"] is matching_Nano_PQ_hip
    rng = np.random.default_rng(2)
    train = rng.standard_normal((40, 8)).astype(np.float32)
    test = rng.standard_normal((3, 8)).astype(np.float32)
    with pytest.raises(ValueError, match="Ks <= 256"):
        matching_Nano_PQ_hip(2, train, test, None, 4, 13)
    with pytest.raises(ValueError, match="Ks <= 256"):
        matching_Nano_PQ_hip(2, train, test, None, 4, 0)
    with pytest.raises(ValueError, match="no multiple of M"):
        matching_Nano_PQ_hip(2, train, test, None, 3, 2)
    with pytest.raises(ValueError, match="n = 40"):
        matching_Nano_PQ_hip(2, train, test, None, 4, 6)
    with pytest.raises(ValueError, match="K = 0"):
        matching_Nano_PQ_hip(0, train, test, None, 4, 2)
    with pytest.raises(ValueError, match="K = 41"):
        matching_Nano_PQ_hip(41, train, test, None, 4, 2)
    with pytest.raises(ValueError, match="K <= 2048"):
        matching_Nano_PQ_hip(2049, np.ones((3000, 8), np.float32), test, None, 4, 2)
    with pytest.raises(ValueError, match="finite and non-zero"):
        matching_Nano_PQ_hip(2, np.where(np.arange(8) == 3, np.nan, train), test, None, 4, 2)
    with pytest.raises(ValueError, match="finite and non-zero"):
        matching_Nano_PQ_hip(2, train, np.zeros((3, 8), np.float32), None, 4, 2)
    with pytest.raises(ValueError, match="expected rows"):
        matching_Nano_PQ_hip(2, train, test[:, :4], None, 4, 2)
    with pytest.raises(ValueError, match="give one"):
        matching_Nano_PQ_hip(2, train, test, None, 4, 2, ifgenerate=False)


def test_missing_codebook_file_is_file_not_found(monkeypatch, tmp_path):
    _refuses(monkeypatch)
    from isehr_amd.nnsearch import matching_Nano_PQ_hip
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(3)
    with pytest.raises(FileNotFoundError):
        matching_Nano_PQ_hip(2, rng.standard_normal((40, 8)), rng.standard_normal((3, 8)), "never/generated", 4, 2, ifgenerate=False)
    assert not os.path.exists(tmp_path / "outputs")


def test_nano_pq_layout_with_a_stubbed_trainer(monkeypatch):
    """Codewords is the inverse of books_of, the reconstruction is the gather codebooks[j, code[:, j]], the trainer sees the
    L2-normalised float32 rows with 20 iterations and seed 42."""
    from isehr_amd import _lib, nnsearch
    rng = np.random.default_rng(4)
    M, Ks, L, n = 4, 8, 3, 50
    books = rng.standard_normal((M, Ks, L)).astype(np.float32)
    codes = rng.integers(0, Ks, size=(n, M)).astype(np.uint8)
    x = rng.standard_normal((n, M * L)) * 7.0
    seen = {}

    class Stub:
        codebooks = books

        def get_codes(self):
            return codes

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            pass

    def fit(rows, m, ks, iters=None, seed=None, **kw):
        seen.update(rows=rows, m=m, ks=ks, iters=iters, seed=seed)
        return Stub()
    monkeypatch.setattr(_lib.PQIndex, "fit", staticmethod(fit))
    got_codes, codewords, recon = nnsearch.Nano_PQ_hip(x, M, Ks)
    assert (seen["m"], seen["ks"], seen["iters"], seen["seed"]) == (M, Ks, 20, 42)
    want_rows = (x / np.expand_dims(np.linalg.norm(x, axis=1), axis=1)).astype(np.float32)
    assert seen["rows"].dtype == np.float32 and np.array_equal(seen["rows"], want_rows)
    assert np.array_equal(got_codes, codes)
    assert codewords.shape == (Ks, M * L) and np.array_equal(books_of(codewords, M), books)
    assert recon.shape == (n, M * L) and recon.dtype == np.float32
    for j in range(M):
        assert np.array_equal(recon[:, j * L:(j + 1) * L], books[j, codes[:, j]])
