"""CPU: the filtered top-K entry point (mi_knn_search_filtered) is exported and bound, rejects bad arguments before touching a
device, the bitmap helpers (allow_bitmap, allow_ranges) pack what they say, and KNN.search without `allow` is the old call."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__
    __graft_entry__.build()
    from isehr_amd import _lib
    return _lib.load(), _lib


def test_symbol_is_exported_and_bound(built_lib):
    lib, _lib = built_lib
    assert hasattr(lib, "mi_knn_search_filtered")
    assert "mi_knn_search_filtered" in _lib.SIGNATURES
    assert lib.mi_knn_search_filtered.restype == C.c_int
    names = [f for f, _ in _lib.FilterInfo._fields_]
    assert names == ["allowed", "path", "kprime", "rerun_queries", "cache_hit"]
    assert C.sizeof(_lib.FilterInfo) == 32


def test_invalid_arguments(built_lib):
    lib, _lib = built_lib
    q = np.zeros((2, 4), np.float32)
    bits = np.zeros(1, np.uint64)
    idx = np.zeros(8, np.int64)
    sc = np.zeros(8, np.float32)
    P = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    fake = C.c_void_p(16)                         # non-null, never dereferenced: every check answers before the handle is read

    def call(g=fake, nq=2, k=4, bitsp=P(bits), memspace=_lib.MI_HOST, dtype=_lib.MI_F32, qp=P(q), out=P(idx)):
        return lib.mi_knn_search_filtered(g, qp, nq, dtype, 4, 1, k, bitsp, memspace, out, P(sc), None, None)

    for kwargs, word in [(dict(g=None), b"null"), (dict(bitsp=None), b"allow_bits"), (dict(memspace=7), b"allow_memspace"),
                         (dict(memspace=-1), b"allow_memspace"), (dict(k=0), b"k must"), (dict(k=2049), b"k must"),
                         (dict(k=-5), b"k must"), (dict(nq=-1), b"nq"), (dict(qp=None), b"queries"),
                         (dict(out=None), b"out_idx"), (dict(dtype=5), b"dtype")]:
        rc = call(**kwargs)
        assert rc == 1, kwargs
        assert word in lib.mi_last_error(), (kwargs, lib.mi_last_error())


def test_allow_bitmap_bit_order(built_lib):
    _, _lib = built_lib
    n = 130
    mask = np.zeros(n, bool)
    mask[[0, 1, 63, 64, 127, 129]] = True
    w = _lib.allow_bitmap(mask, n)
    assert w.dtype == np.dtype("<u8") and w.shape == (3,)
    assert int(w[0]) == (1 << 0) | (1 << 1) | (1 << 63)
    assert int(w[1]) == (1 << 0) | (1 << 63)
    assert int(w[2]) == 1 << 1
    # the same from ids, from packed words, and the reference decoding: bit (i & 63) of word (i >> 6)
    ids = np.flatnonzero(mask)
    assert (_lib.allow_bitmap(ids, n) == w).all()
    assert (_lib.allow_bitmap(w, n) == w).all()
    dec = np.array([(int(w[i >> 6]) >> (i & 63)) & 1 for i in range(n)], bool)
    assert (dec == mask).all()


def test_bits_beyond_n_are_ignored(built_lib):
    _, _lib = built_lib
    n = 70
    words = np.array([0, 0xFFFFFFFFFFFFFFFF], np.uint64)          # rows 64..69 allowed, bits 70..127 set but outside the shard
    w = _lib.allow_bitmap(words, n, packed=True)
    valid = np.array([(int(w[i >> 6]) >> (i & 63)) & 1 for i in range(n)], bool)
    assert valid.sum() == 6 and valid[64:].all()
    # what the library counts: the host popcount of the masked words (mirrors api_filter.hip)
    masked = w.copy()
    masked[-1] &= np.uint64((1 << (n % 64)) - 1)
    assert sum(bin(int(x)).count("1") for x in masked) == 6
    # a packed mask never sets a bit at or beyond n
    full = _lib.allow_bitmap(np.ones(n, bool), n)
    assert int(full[1]) == (1 << 6) - 1


def test_ids_made_local_by_row_offset(built_lib):
    _, _lib = built_lib
    n, off = 100, 1_000_000
    w = _lib.allow_bitmap(np.array([off, off + 5, off + 99]), n, row_offset=off)
    assert int(w[0]) == 1 | (1 << 5) and int(w[1]) == 1 << 35
    with pytest.raises(ValueError):
        _lib.allow_bitmap(np.array([off - 1]), n, row_offset=off)      # below the shard
    with pytest.raises(ValueError):
        _lib.allow_bitmap(np.array([off + 100]), n, row_offset=off)    # beyond it
    with pytest.raises(ValueError):
        _lib.allow_bitmap(np.array([5]), n, row_offset=off)            # a local id is not a global one here
    with pytest.raises(ValueError):
        _lib.allow_bitmap(np.ones(n + 1, bool), n)
    with pytest.raises(ValueError):
        _lib.allow_bitmap(np.zeros(3, np.uint64), n, packed=True)


def test_packed_words_are_never_guessed(built_lib):
    _, _lib = built_lib
    n = 128                                                          # two words
    # a plain uint64 array of two entries is two ids, not two words
    w = _lib.allow_bitmap(np.array([3, 70], np.uint64), n)
    assert isinstance(w, _lib.AllowBits)
    assert int(w[0]) == 1 << 3 and int(w[1]) == 1 << 6
    # the helpers' own output passes through unchanged, words given explicitly too
    assert (_lib.allow_bitmap(w, n) == w).all() and isinstance(_lib.allow_bitmap(w, n), _lib.AllowBits)
    raw = np.array([5, 0], np.uint64)
    assert (_lib.allow_bitmap(raw, n, packed=True) == raw).all()
    with pytest.raises(ValueError):
        _lib.allow_bitmap(w, 200)                                    # words of another shard size
    # an empty id list allows nothing
    for empty in ([], np.array([], np.int64), ()):
        e = _lib.allow_bitmap(empty, n)
        assert e.shape == (2,) and not e.any()


def test_allow_ranges(built_lib):
    _, _lib = built_lib
    n = 300
    w = _lib.allow_ranges([(0, 10), (100, 200), (290, 400)], n)
    got = np.array([(int(w[i >> 6]) >> (i & 63)) & 1 for i in range(n)], bool)
    want = np.zeros(n, bool)
    want[:10] = want[100:200] = want[290:] = True
    assert (got == want).all()
    # a shard at row_offset 1000 of a concatenation: only the part of each range inside the shard
    w2 = _lib.allow_ranges([(900, 1010), (1250, 5000)], 100 + 200, row_offset=1000)
    got2 = np.array([(int(w2[i >> 6]) >> (i & 63)) & 1 for i in range(300)], bool)
    want2 = np.zeros(300, bool)
    want2[:10] = want2[250:] = True
    assert (got2 == want2).all()
    with pytest.raises(ValueError):
        _lib.allow_ranges([(5, 2)], n)
    with pytest.raises(ValueError):
        _lib.allow_ranges([(-1, 2)], n)


def test_knn_search_without_allow_is_the_old_call(built_lib, monkeypatch):
    _, _lib = built_lib
    from isehr_amd.knn import KNN
    calls = []

    class FakeGallery:
        def search(self, q, k):
            calls.append(("search", q.dtype, q.shape, k))
            return np.zeros((q.shape[0], k), np.int64) + 3, np.ones((q.shape[0], k), np.float32), 0.0

        def search_filtered(self, q, k, allow):
            calls.append(("search_filtered", q.dtype, q.shape, k, allow))
            return np.zeros((q.shape[0], k), np.int64) - 1, np.full((q.shape[0], k), -np.inf, np.float32), 0.0, {}

    knn = object.__new__(KNN)
    knn.gallery = FakeGallery()
    knn.N, knn.D = 10, 4
    sims, ids = knn.search(np.zeros((2, 4), np.float64), 5)
    assert calls == [("search", np.float32, (2, 4), 5)]
    assert (ids == 3).all() and (sims == 1).all()
    sims, ids = knn.search(np.zeros((2, 4), np.float32), 5, allow=None)
    assert calls[-1][0] == "search" and len(calls) == 2
    allow = np.array([1, 2])
    sims, ids = knn.search(np.zeros((2, 4), np.float32), 5, allow=allow)
    assert calls[-1][0] == "search_filtered" and calls[-1][4] is allow
    assert (ids == -1).all() and np.isneginf(sims).all()


def test_gallery_search_filtered_needs_one_bitmap(built_lib):
    _, _lib = built_lib
    g = object.__new__(_lib.Gallery)
    g.n, g.d, g.row_offset = 10, 4, 0
    with pytest.raises(ValueError):
        g.search_filtered(np.zeros((1, 4), np.float32), 3)
    with pytest.raises(ValueError):
        g.search_filtered(np.zeros((1, 4), np.float32), 3, allow=np.ones(10, bool), allow_ptr=1234)
