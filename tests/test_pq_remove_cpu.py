"""CPU: the surface of mi_pq_remove_rows / mi_ivfpq_remove_rows (include/mi355_retrieval.h, csrc/api_pq.hip, csrc/api_ivfpq.hip)
without a device -- the argument checks that answer before any device is touched, the global option "pq_remove_block_rows", and
what PQIndex.remove / IVFPQIndex.remove / ANN.remove_ids do around the call, on a stub that needs no handle."""
import ctypes as C
import os
import re
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ["mi_pq_remove_rows", "mi_ivfpq_remove_rows"]
HANDLE = {"mi_pq_remove_rows": "mi_pq* h", "mi_ivfpq_remove_rows": "mi_ivfpq* h"}


@pytest.fixture(scope="module")
def built():
    import __graft_entry__
    __graft_entry__.build()
    from isehr_amd import _lib
    return _lib.load(), _lib


@pytest.mark.parametrize("name", ENTRY)
def test_header_declares_and_library_exports_the_symbol(built, name):
    lib, _lib = built
    hdr = open(os.path.join(ROOT, "include", "mi355_retrieval.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"int\s+%s\s*\(([^)]*)\)\s*;" % name, code)
    assert m, "the header does not declare " + name
    args = [a.strip() for a in m.group(1).split(",")]
    assert args == [HANDLE[name], "const uint64_t* remove_bits", "int memspace", "int64_t* out_removed"], args
    assert hasattr(lib, name)
    res, argtypes = _lib.SIGNATURES[name]
    assert res is C.c_int and len(argtypes) == 4


@pytest.mark.parametrize("name", ENTRY)
def test_argument_checks_answer_before_any_device_is_touched(built, name):
    lib, _lib = built
    call = getattr(lib, name)
    bits = np.zeros(4, np.uint64)
    fake = C.c_void_p(0x1000)              # never dereferenced: the checks below fail first
    removed = C.c_int64(0)
    rc = call(None, C.c_void_p(bits.ctypes.data), _lib.MI_HOST, C.byref(removed))
    assert rc == 1 and b"null handle" in lib.mi_last_error() and removed.value == 0
    rc = call(fake, None, _lib.MI_HOST, C.byref(removed))
    assert rc == 1 and b"remove_bits" in lib.mi_last_error() and removed.value == 0
    for bad in (5, -1, 2):
        rc = call(fake, C.c_void_p(bits.ctypes.data), bad, C.byref(removed))
        assert rc == 1 and b"memspace" in lib.mi_last_error() and removed.value == 0
    assert call(fake, None, _lib.MI_HOST, None) == 1                     # out_removed may be NULL on every path
    with pytest.raises(RuntimeError, match="null handle"):
        _lib.check(call(None, C.c_void_p(bits.ctypes.data), _lib.MI_HOST, None))


def test_pq_remove_block_rows_is_a_global_option_of_at_least_64_rows(built):
    lib, _lib = built
    default = _lib.get_global_option("pq_remove_block_rows")
    assert default == 2 ** 21
    try:
        for value, stored in ((64, 64), (65, 128), (4096, 4096), (100000, 100032)):
            _lib.set_global_option("pq_remove_block_rows", value)
            assert _lib.get_global_option("pq_remove_block_rows") == stored
        for bad in (63.0, 1.0, -1.0, -64.0):
            assert lib.mi_set_global_option(b"pq_remove_block_rows", bad) == 1
            assert b"pq_remove_block_rows" in lib.mi_last_error()
            assert _lib.get_global_option("pq_remove_block_rows") == 100032      # a refused value changes nothing
    finally:
        _lib.set_global_option("pq_remove_block_rows", 0)                        # 0 = default
    assert _lib.get_global_option("pq_remove_block_rows") == default
    assert _lib.get_global_option("remove_block_rows") == 0                      # the gallery's option is another one


class _StubLib:
    """Stands in for the loaded library: records the bitmap of the call and answers like the two entry points."""

    def __init__(self, n, lie=0):
        self.n, self.lie, self.calls = n, lie, []

    def _remove(self, name, h, bits_p, memspace, out_removed):
        nwords = max(1, (self.n + 63) // 64)
        words = np.ctypeslib.as_array(C.cast(bits_p, C.POINTER(C.c_uint64)), shape=(nwords,)).copy()
        gone = np.unpackbits(words.view(np.uint8), bitorder="little")[:self.n]
        self.calls.append((name, words, memspace))
        out_removed._obj.value = int(gone.sum()) + self.lie
        self.n -= int(gone.sum())
        return 0

    def mi_pq_remove_rows(self, *a):
        return self._remove("mi_pq_remove_rows", *a)

    def mi_ivfpq_remove_rows(self, *a):
        return self._remove("mi_ivfpq_remove_rows", *a)


KINDS = [("PQIndex", "mi_pq_remove_rows"), ("IVFPQIndex", "mi_ivfpq_remove_rows")]


def _stub_index(_lib, monkeypatch, cls, n, row_offset=0, lie=0):
    stub = _StubLib(n, lie)
    monkeypatch.setattr(_lib, "load", lambda: stub)
    idx = getattr(_lib, cls).__new__(getattr(_lib, cls))
    idx._h, idx._lock = None, threading.Lock()         # _h None: close() / __del__ have nothing to destroy
    idx.n, idx.d, idx.m, idx.ks, idx.row_offset = n, 8, 2, 16, row_offset
    return idx, stub


@pytest.mark.parametrize("cls,entry", KINDS)
@pytest.mark.parametrize("row_offset", [0, 2 ** 33])
def test_remove_kept_array_for_mask_ids_and_packed_words(built, monkeypatch, cls, entry, row_offset):
    _, _lib = built
    n = 1500
    rng = np.random.default_rng(5)
    mask = rng.random(n) < 0.3
    mask[[0, 63, 64, n - 1]] = True
    want_kept = np.flatnonzero(~mask).astype(np.int64) + row_offset
    ids = np.flatnonzero(mask).astype(np.int64) + row_offset
    ids_dup = np.concatenate([ids[::-1], ids[:17]])                      # unordered, with duplicates
    packed = _lib.allow_bitmap(mask, n)
    ref_words = None
    for rows in (mask, ids, ids_dup, ids.astype(np.uint64), packed):
        idx, stub = _stub_index(_lib, monkeypatch, cls, n, row_offset)
        kept = idx.remove(rows)
        assert kept.dtype == np.int64 and np.array_equal(kept, want_kept)
        assert idx.n == n - int(mask.sum()) == kept.size
        (name, words, memspace), = stub.calls
        assert name == entry and memspace == _lib.MI_HOST
        if ref_words is None:
            ref_words = words
            got = np.unpackbits(words.view(np.uint8), bitorder="little")
            assert np.array_equal(got[:n].astype(bool), mask) and not got[n:].any()   # local rows, nothing beyond n
        assert np.array_equal(words, ref_words)
    idx, stub = _stub_index(_lib, monkeypatch, cls, n, row_offset)           # nothing named: everything is kept
    kept = idx.remove(np.zeros(0, np.int64))
    assert np.array_equal(kept, np.arange(n) + row_offset) and idx.n == n
    idx, stub = _stub_index(_lib, monkeypatch, cls, n, row_offset)           # everything named
    kept = idx.remove(np.ones(n, bool))
    assert kept.size == 0 and kept.dtype == np.int64 and idx.n == 0
    kept = idx.remove(np.zeros(0, bool))                                     # an empty index takes the call as well
    assert kept.size == 0 and idx.n == 0


@pytest.mark.parametrize("cls,entry", KINDS)
def test_remove_refuses_ids_outside_the_shard_before_the_call(built, monkeypatch, cls, entry):
    _, _lib = built
    off = 1000
    for bad in ([off - 1], [off + 300], [off, off + 5, 5], [-1], np.array([2 ** 63], np.uint64)):
        idx, stub = _stub_index(_lib, monkeypatch, cls, 300, off)
        with pytest.raises(ValueError):
            idx.remove(bad)
        assert stub.calls == [] and idx.n == 300
    idx, stub = _stub_index(_lib, monkeypatch, cls, 300, off)
    with pytest.raises(ValueError):
        idx.remove(np.zeros(299, bool))                                      # mask of the wrong length
    with pytest.raises(ValueError):
        idx.remove(np.zeros(4, np.uint64).view(_lib.AllowBits))              # 300 rows take 5 words
    assert stub.calls == [] and idx.n == 300


@pytest.mark.parametrize("cls,entry", KINDS)
def test_remove_raises_when_the_library_counts_otherwise(built, monkeypatch, cls, entry):
    _, _lib = built
    idx, stub = _stub_index(_lib, monkeypatch, cls, 100, lie=1)
    with pytest.raises(RuntimeError, match=entry):
        idx.remove([3, 4])
    assert idx.n == 100


def test_ann_remove_ids_passes_through_to_the_index(built):
    _, _lib = built
    from isehr_amd.knn import ANN, KNN

    class FakeIndex:
        def __init__(self, n):
            self.n, self.calls = n, []

        def remove(self, rows):
            self.calls.append(rows)
            gone = np.unique(np.asarray(rows, np.int64))
            self.n -= gone.size
            return np.setdiff1d(np.arange(self.n + gone.size), gone)

    ann = ANN.__new__(ANN)
    ann.index, ann.N, ann.D, ann.method, ann.nprobe = FakeIndex(100), 100, 8, "euclidean", 4
    ids = np.array([3, 3, 99, 0])
    assert ann.remove_ids(ids) == 3
    assert ann.N == 97 and ann.index.n == 97 and ann.index.calls[0] is ids
    assert ann.remove_ids([]) == 0 and ann.N == 97
    # binary indexes stay without removal
    knn = KNN.__new__(KNN)
    knn.method = "hamming"
    with pytest.raises(NotImplementedError):
        knn.remove_ids([0])
