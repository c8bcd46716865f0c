"""CPU: the surface of mi_gallery_remove_rows (include/mi355_retrieval.h, csrc/api_remove.hip) without a device -- the symbol, the
argument checks that answer before any device is touched, the global option, and what Gallery.remove / KNN.remove_ids do around
the call (id validation, the `kept` array), on a stub that needs no handle."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__
    __graft_entry__.build()
    from isehr_amd import _lib
    return _lib.load(), _lib


def test_header_declares_and_library_exports_the_symbol(built):
    lib, _lib = built
    hdr = open(os.path.join(ROOT, "include", "mi355_retrieval.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"int\s+mi_gallery_remove_rows\s*\(([^)]*)\)\s*;", code)
    assert m, "the header does not declare mi_gallery_remove_rows"
    args = [a.strip() for a in m.group(1).split(",")]
    assert args == ["mi_gallery* g", "const uint64_t* remove_bits", "int memspace", "int64_t* out_removed"], args
    assert hasattr(lib, "mi_gallery_remove_rows")
    res, argtypes = _lib.SIGNATURES["mi_gallery_remove_rows"]
    assert res is C.c_int and len(argtypes) == 4


def test_argument_checks_answer_before_any_device_is_touched(built):
    lib, _lib = built
    bits = np.zeros(4, np.uint64)
    removed = C.c_int64(-7)
    fake = C.c_void_p(0x1000)              # never dereferenced: the checks below fail first
    rc = lib.mi_gallery_remove_rows(None, C.c_void_p(bits.ctypes.data), _lib.MI_HOST, C.byref(removed))
    assert rc == 1 and b"null handle" in lib.mi_last_error()
    rc = lib.mi_gallery_remove_rows(fake, None, _lib.MI_HOST, None)
    assert rc == 1 and b"remove_bits" in lib.mi_last_error()
    for bad in (-1, 2, 99):
        rc = lib.mi_gallery_remove_rows(fake, C.c_void_p(bits.ctypes.data), bad, None)
        assert rc == 1 and b"memspace" in lib.mi_last_error()
    with pytest.raises(RuntimeError, match="null handle"):
        _lib.check(lib.mi_gallery_remove_rows(None, C.c_void_p(bits.ctypes.data), _lib.MI_HOST, None))


def test_remove_block_rows_is_a_global_option_rounded_up_to_whole_tiles(built):
    lib, _lib = built
    assert _lib.get_global_option("remove_block_rows") == 0
    try:
        _lib.set_global_option("remove_block_rows", 256)
        assert _lib.get_global_option("remove_block_rows") == 256
        _lib.set_global_option("remove_block_rows", 257)
        assert _lib.get_global_option("remove_block_rows") == 512
        _lib.set_global_option("remove_block_rows", 4096)
        assert _lib.get_global_option("remove_block_rows") == 4096
    finally:
        _lib.set_global_option("remove_block_rows", 0)
    assert _lib.get_global_option("remove_block_rows") == 0
    assert lib.mi_set_global_option(b"remove_block_rows", -1.0) == 1 and b"remove_block_rows" in lib.mi_last_error()


class _StubLib:
    """Stands in for the loaded library: records the bitmap of the call and answers like mi_gallery_remove_rows."""

    def __init__(self, n):
        self.n, self.calls = n, []

    def mi_gallery_remove_rows(self, h, bits_p, memspace, out_removed):
        nwords = (self.n + 63) // 64
        words = np.ctypeslib.as_array(C.cast(bits_p, C.POINTER(C.c_uint64)), shape=(nwords,)).copy()
        gone = np.unpackbits(words.view(np.uint8), bitorder="little")[:self.n]
        self.calls.append((words, memspace))
        out_removed._obj.value = int(gone.sum())
        self.n -= int(gone.sum())
        return 0


def _stub_gallery(_lib, monkeypatch, n, row_offset=0):
    import threading
    stub = _StubLib(n)
    monkeypatch.setattr(_lib, "load", lambda: stub)
    g = _lib.Gallery.__new__(_lib.Gallery)
    g._h, g._lock = None, threading.Lock()           # _h None: close() / __del__ have nothing to destroy
    g.n, g.d, g.row_offset = n, 8, row_offset
    return g, stub


@pytest.mark.parametrize("row_offset", [0, 2 ** 33])
def test_gallery_remove_kept_array_for_mask_ids_and_packed_words(built, monkeypatch, row_offset):
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
        g, stub = _stub_gallery(_lib, monkeypatch, n, row_offset)
        kept = g.remove(rows)
        assert kept.dtype == np.int64 and np.array_equal(kept, want_kept)
        assert g.n == n - int(mask.sum()) == kept.size
        (words, memspace), = stub.calls
        assert memspace == _lib.MI_HOST
        if ref_words is None:
            ref_words = words
            got = np.unpackbits(words.view(np.uint8), bitorder="little")
            assert np.array_equal(got[:n].astype(bool), mask) and not got[n:].any()   # local rows, nothing beyond n
        assert np.array_equal(words, ref_words)
    g, stub = _stub_gallery(_lib, monkeypatch, n, row_offset)                # nothing named: everything is kept
    kept = g.remove(np.zeros(0, np.int64))
    assert np.array_equal(kept, np.arange(n) + row_offset) and g.n == n
    g, stub = _stub_gallery(_lib, monkeypatch, n, row_offset)                # everything named
    kept = g.remove(np.ones(n, bool))
    assert kept.size == 0 and kept.dtype == np.int64 and g.n == 0


def test_gallery_remove_refuses_ids_outside_the_shard_before_the_call(built, monkeypatch):
    _, _lib = built
    off = 1000
    for bad in ([off - 1], [off + 300], [off, off + 5, 5], [-1], np.array([2 ** 63], np.uint64)):
        g, stub = _stub_gallery(_lib, monkeypatch, 300, off)
        with pytest.raises(ValueError):
            g.remove(bad)
        assert stub.calls == [] and g.n == 300
    g, stub = _stub_gallery(_lib, monkeypatch, 300, off)
    with pytest.raises(ValueError):
        g.remove(np.zeros(299, bool))                                        # mask of the wrong length
    with pytest.raises(ValueError):
        g.remove(np.zeros(4, np.uint64).view(_lib.AllowBits))                # 300 rows take 5 words
    assert stub.calls == []


def test_knn_remove_ids_returns_the_number_removed(built, monkeypatch):
    _, _lib = built
    from isehr_amd.knn import KNN
    g, stub = _stub_gallery(_lib, monkeypatch, 100)
    knn = KNN.__new__(KNN)
    knn.gallery, knn.N, knn.D, knn.method = g, 100, 8, "euclidean"
    assert knn.remove_ids(np.array([3, 3, 99, 0])) == 3
    assert knn.N == 97 and g.n == 97
    assert knn.remove_ids([]) == 0 and knn.N == 97
