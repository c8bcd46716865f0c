"""CPU: the range-search entry point (mi_range_search) is exported and bound, rejects bad arguments before touching a device,
and the host-side logic around it -- the capacity retry of Gallery.range_search, the pair selection of near_duplicate_pairs --
does what it says against a fake library that returns canned CSR results."""
import ctypes as C
import threading

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
    assert hasattr(lib, "mi_range_search")
    assert "mi_range_search" in _lib.SIGNATURES
    assert lib.mi_range_search.restype == C.c_int
    assert _lib.MI_ERR_CAPACITY == 7


def test_invalid_arguments(built_lib):
    lib, _lib = built_lib
    q = np.zeros((2, 4), np.float32)
    lims = np.zeros(3, np.int64)
    idx = np.zeros(8, np.int64)
    sc = np.zeros(8, np.float32)
    P = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    # null gallery
    rc = lib.mi_range_search(None, P(q), 2, _lib.MI_F32, 4, 1, 0.5, 8, P(lims), P(idx), P(sc), None)
    assert rc == 1 and b"null" in lib.mi_last_error()
    # nq < 0 and null out_lims, with a non-null (never dereferenced) handle
    fake = C.c_void_p(16)
    rc = lib.mi_range_search(fake, P(q), -1, _lib.MI_F32, 4, 1, 0.5, 8, P(lims), P(idx), P(sc), None)
    assert rc == 1 and b"nq" in lib.mi_last_error()
    rc = lib.mi_range_search(fake, P(q), 2, _lib.MI_F32, 4, 1, 0.5, 8, None, P(idx), P(sc), None)
    assert rc == 1 and b"out_lims" in lib.mi_last_error()


class _FakeLib:
    """mi_range_search returning canned CSR results per query row (row i of the query array carries its query id in
    column 0).  hits: {query id: [(id, score), ...]} already in (score desc, id asc) order."""

    def __init__(self, hits):
        self.hits = hits
        self.calls = []

    def mi_range_search(self, h, qptr, nq, code, rs, cs, min_score, cap, lims_p, idx_p, sc_p, secs_p):
        q = np.ctypeslib.as_array(C.cast(qptr, C.POINTER(C.c_float)), shape=(nq, rs))
        lims = np.ctypeslib.as_array(C.cast(lims_p, C.POINTER(C.c_int64)), shape=(nq + 1,))
        per = [self.hits.get(int(q[i, 0]), []) for i in range(nq)]
        self.calls.append(cap)
        lims[0] = 0
        for i, p in enumerate(per):
            lims[i + 1] = lims[i] + len(p)
        if lims[-1] > cap:
            return 7
        if cap:
            idx = np.ctypeslib.as_array(C.cast(idx_p, C.POINTER(C.c_int64)), shape=(cap,))
            sc = np.ctypeslib.as_array(C.cast(sc_p, C.POINTER(C.c_float)), shape=(cap,))
            flat = [e for p in per for e in p]
            for j, (i_, s_) in enumerate(flat):
                idx[j], sc[j] = i_, s_
        return 0

    def mi_last_error(self):
        return b"fake"


def _fake_gallery(monkeypatch, _lib, hits, n=10, d=4):
    fake = _FakeLib(hits)
    monkeypatch.setattr(_lib, "load", lambda: fake)
    g = object.__new__(_lib.Gallery)
    g._h = C.c_void_p(1)
    g._lock = threading.Lock()
    g.n, g.d, g.norm_mode, g.device, g.row_offset, g.hbm_bytes = n, d, 1, 0, 0, 0
    g.get_rows = lambda r0, m: np.array([[r0 + i] + [0] * (d - 1) for i in range(m)], np.float32)
    monkeypatch.setattr(_lib.Gallery, "__del__", lambda self: None)
    return g, fake


def test_capacity_retry_once(built_lib, monkeypatch):
    _, _lib = built_lib
    hits = {0: [(3, 0.9), (5, 0.8), (1, 0.7)], 1: [(2, 0.95)]}
    g, fake = _fake_gallery(monkeypatch, _lib, hits)
    q = np.array([[0, 0, 0, 0], [1, 0, 0, 0]], np.float32)
    lims, idx, sc, _ = g.range_search(q, 0.5, max_results=2)
    assert fake.calls == [2, 4]                       # first guess, then exactly lims[-1]
    assert lims.tolist() == [0, 3, 4]
    assert idx.tolist() == [3, 5, 1, 2]
    assert np.allclose(sc, [0.9, 0.8, 0.7, 0.95])
    # ample capacity: no retry; default guess nq * 1024
    fake.calls.clear()
    lims2, idx2, sc2, _ = g.range_search(q, 0.5)
    assert fake.calls == [2 * 1024]
    assert lims2.tolist() == lims.tolist() and idx2.tolist() == idx.tolist()


def test_capacity_error_is_raised_when_the_retry_fails_too(built_lib, monkeypatch):
    _, _lib = built_lib
    g, fake = _fake_gallery(monkeypatch, _lib, {0: [(1, 0.9), (2, 0.8)]})
    orig = fake.mi_range_search
    fake.mi_range_search = lambda *a: (orig(*a), 7)[1]       # never satisfied
    with pytest.raises(RuntimeError):
        g.range_search(np.zeros((1, 4), np.float32), 0.5, max_results=1)
    assert len(fake.calls) == 2                                # one retry only


def test_near_duplicate_pairs_selection(built_lib, monkeypatch):
    _, _lib = built_lib
    from isehr_amd.dedup import near_duplicate_pairs
    # symmetric duplicate groups {0, 4, 7} and {2, 3}; every query finds itself too
    hits = {0: [(0, 1.0), (4, 0.99), (7, 0.98)], 4: [(4, 1.0), (0, 0.99), (7, 0.97)], 7: [(7, 1.0), (0, 0.98), (4, 0.97)],
            2: [(2, 1.0), (3, 0.96)], 3: [(3, 1.0), (2, 0.96)]}
    g, fake = _fake_gallery(monkeypatch, _lib, hits, n=10)
    i, j, s = near_duplicate_pairs(g, 0.95, batch=3)
    got = sorted(zip(i.tolist(), j.tolist()))
    assert got == [(0, 4), (0, 7), (2, 3), (4, 7)]            # i < j, each pair once, no self pairs
    assert (i < j).all()
    assert i.dtype == np.int64 and j.dtype == np.int64 and s.dtype == np.float32
    byp = dict(zip(zip(i.tolist(), j.tolist()), s.tolist()))
    assert byp[(4, 7)] == pytest.approx(0.97)                  # the score of row i's query
    assert len(fake.calls) == 4                                # ceil(10 / 3) range searches


def test_near_duplicate_pairs_refuses_offset_galleries(built_lib, monkeypatch):
    _, _lib = built_lib
    from isehr_amd.dedup import near_duplicate_pairs
    g, _ = _fake_gallery(monkeypatch, _lib, {})
    g.row_offset = 5
    with pytest.raises(ValueError):
        near_duplicate_pairs(g, 0.9)
