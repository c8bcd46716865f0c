"""CPU: the plumbing every index class of the binding shares (_lib._Handle, _resolve_allow, _range_call), on stand-ins for the
loaded library: nothing here needs a device or the built library."""
import ctypes as C
import threading

import numpy as np
import pytest

from isehr_amd import _lib


class _FakeLib:
    """Stands in for the loaded library: a destroy function that answers with the next code of `codes` (0 once they run out)."""

    def __init__(self, codes=()):
        self.codes, self.destroyed = list(codes), []

    def fake_destroy(self, h):
        self.destroyed.append(h.value)
        return self.codes.pop(0) if self.codes else 0

    def mi_last_error(self):
        return b"an online chain is still built on the gallery"


class _Thing(_lib._Handle):
    _DESTROY = "fake_destroy"


def test_close_destroys_exactly_once(monkeypatch):
    fake = _FakeLib()
    monkeypatch.setattr(_lib, "load", lambda: fake)
    with _Thing(0x1234) as t:
        assert t._h.value == 0x1234 and t._lock.acquire(False)
        t._lock.release()
    assert fake.destroyed == [0x1234] and t._h is None
    t.close()
    t.close()
    assert fake.destroyed == [0x1234]
    _Thing(0).close()                                   # a null handle is never handed to the library
    assert fake.destroyed == [0x1234]


def test_refused_destroy_raises_and_keeps_the_handle(monkeypatch):
    fake = _FakeLib([3])
    monkeypatch.setattr(_lib, "load", lambda: fake)
    t = _Thing(77)
    with pytest.raises(RuntimeError, match="error 3: an online chain is still built"):
        t.close()
    assert t._h is not None and t._h.value == 77
    t.close()                                           # the later close tries again, and is let through
    assert fake.destroyed == [77, 77] and t._h is None


def test_del_swallows_a_refused_destroy(monkeypatch):
    fake = _FakeLib([3, 3])
    monkeypatch.setattr(_lib, "load", lambda: fake)
    t = _Thing(5)
    t.__del__()
    assert fake.destroyed == [5] and t._h.value == 5
    with pytest.raises(RuntimeError):
        t.__exit__(None, None, None)                    # (the `with` exit does not swallow it)
    t.close()
    half_made = _Thing.__new__(_Thing)                  # __init__ never ran: no _h at all
    half_made.__del__()


def test_every_handle_class_is_a_context_manager_with_one_close():
    for cls in (_lib.Gallery, _lib.BinaryGallery, _lib.PQIndex, _lib.IVFPQIndex, _lib.GraphIndex, _lib.PQGraphIndex, _lib.OnlineChain):
        assert issubclass(cls, _lib._Handle), cls
        assert cls.close is _lib._Handle.close and cls.__del__ is _lib._Closing.__del__, cls
        assert cls._DESTROY in _lib.SIGNATURES and cls._DESTROY.endswith("_destroy"), cls
    for cls in (_lib.Gallery, _lib.BinaryGallery, _lib.LSHIndex):
        assert hasattr(cls, "__enter__") and hasattr(cls, "__exit__"), cls
    assert _lib.LSHIndex.close is not _lib._Handle.close and _lib.LSHIndex.__del__ is _lib._Closing.__del__


def test_hbm_bytes_asks_the_info_call_for_its_last_output_only(monkeypatch):
    seen = {}

    class Info:
        def __getattr__(self, name):
            def info(h, *outs):
                seen[name] = outs[:-1]
                outs[-1].value = 4096
                return 0
            return info

    monkeypatch.setattr(_lib, "load", lambda: Info())
    for cls, name in ((_lib.BinaryGallery, "mi_hamming_info"), (_lib.PQIndex, "mi_pq_info"), (_lib.IVFPQIndex, "mi_ivfpq_info"),
                      (_lib.PQGraphIndex, "mi_pq_graph_info")):
        obj = cls.__new__(cls)
        obj._h = None
        assert obj.hbm_bytes == 4096
        # the handle and the trailing hbm_bytes are the only arguments in use: one None for each other argument of the C call
        assert seen[name] == (None,) * (len(_lib.SIGNATURES[name][1]) - 2), name


def _bits_of(words, n):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:n].astype(bool)


def test_resolve_allow_without_an_allow_list():
    assert _lib._resolve_allow(None, None, 10, 0) == (None, None, _lib.MI_HOST)


@pytest.mark.parametrize("n", [1, 64, 65])
def test_resolve_allow_packs_a_mask_into_host_words(n):
    mask = np.zeros(n, bool)
    mask[[0, n - 1, n // 2]] = True
    keep, ptr, memspace = _lib._resolve_allow(mask, None, n, 0)
    assert memspace == _lib.MI_HOST and keep.dtype == np.uint64 and keep.shape == ((n + 63) // 64,)
    assert isinstance(ptr, C.c_void_p) and ptr.value == keep.ctypes.data
    assert np.array_equal(_bits_of(keep, n), mask)
    assert not np.unpackbits(keep.view(np.uint8), bitorder="little")[n:].any()            # the padding bits stay clear
    # global ids of a shard at an offset give the same words
    keep2, _, _ = _lib._resolve_allow(np.flatnonzero(mask) + 1000, None, n, 1000)
    assert np.array_equal(keep2, keep)


def test_resolve_allow_gives_an_empty_bitmap_one_zero_word():
    keep, ptr, memspace = _lib._resolve_allow(np.zeros(0, bool), None, 0, 0)
    assert keep.dtype == np.uint64 and keep.tolist() == [0] and ptr.value == keep.ctypes.data and memspace == _lib.MI_HOST
    assert _lib._allow_words(np.zeros(0, bool), 0, 0).tolist() == [0] and _lib._allow_words(None, 0, 0) is None


def test_resolve_allow_passes_a_device_pointer_on():
    keep, ptr, memspace = _lib._resolve_allow(None, 12345, 10, 0)
    assert keep is None and isinstance(ptr, C.c_void_p) and ptr.value == 12345 and memspace == _lib.MI_DEVICE


def test_resolve_allow_refuses_both():
    with pytest.raises(ValueError, match="^give at most one of allow and allow_ptr$"):
        _lib._resolve_allow(np.ones(4, bool), 12345, 4, 0)
    with pytest.raises(ValueError, match="allowed ids must lie in"):
        _lib._resolve_allow([4], None, 4, 0)


class _RangeCall:
    """A range call of `total` hits (ids 0 .. total - 1, values 10 * id): answers MI_ERR_CAPACITY below that capacity, or always
    with stubborn=True.  lims is written either way, ids and values only when they fit."""

    def __init__(self, nq, total, ctype, stubborn=False):
        self.nq, self.total, self.ctype, self.stubborn, self.caps = nq, total, ctype, stubborn, []

    def __call__(self, cap, lims_p, idx_p, val_p, secs_p):
        self.caps.append(cap)
        lims = np.ctypeslib.as_array(C.cast(lims_p, C.POINTER(C.c_int64)), shape=(self.nq + 1,))
        lims[:] = 0
        lims[-1] = self.total
        if self.stubborn or self.total > cap:
            return _lib.MI_ERR_CAPACITY
        if self.total:
            np.ctypeslib.as_array(C.cast(idx_p, C.POINTER(C.c_int64)), shape=(cap,))[:self.total] = np.arange(self.total)
            np.ctypeslib.as_array(C.cast(val_p, C.POINTER(self.ctype)), shape=(cap,))[:self.total] = 10 * np.arange(self.total)
        secs_p._obj.value = 0.25
        return 0


@pytest.mark.parametrize("dtype,ctype", [(np.float32, C.c_float), (np.int32, C.c_int32)])
def test_range_call_retries_once_with_exactly_the_reported_total(dtype, ctype):
    call = _RangeCall(2, 7, ctype)
    lock = threading.Lock()
    lims, idx, val, secs = _lib._range_call(lock, call, 2, 3, dtype)
    assert call.caps == [3, 7]
    assert lims.dtype == np.int64 and lims.tolist() == [0, 0, 7]
    assert idx.dtype == np.int64 and idx.tolist() == list(range(7))
    assert val.dtype == dtype and val.tolist() == [10 * i for i in range(7)]
    assert secs == 0.25 and not lock.locked()


def test_range_call_raises_when_the_retry_does_not_fit_either(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: _FakeLib())
    call = _RangeCall(1, 7, C.c_float, stubborn=True)
    lock = threading.Lock()
    with pytest.raises(RuntimeError, match="error %d" % _lib.MI_ERR_CAPACITY):
        _lib._range_call(lock, call, 1, 3, np.float32)
    assert call.caps == [3, 7] and not lock.locked()


def test_range_call_that_fits_is_made_once_and_defaults_to_1024_per_query():
    call = _RangeCall(3, 5, C.c_int32)
    lims, idx, val, _ = _lib._range_call(threading.Lock(), call, 3, None, np.int32)
    assert call.caps == [3 * 1024] and idx.shape == val.shape == (5,) and lims[-1] == 5
    assert _lib._range_capacity(3, None) == 3 * 1024 and _lib._range_capacity(3, 17) == 17 and _lib._range_capacity(0, None) == 0
    call = _RangeCall(1, 0, C.c_int32)                  # capacity 0 and no hits: one call, empty answers
    lims, idx, val, _ = _lib._range_call(threading.Lock(), call, 1, 0, np.int32)
    assert call.caps == [0] and idx.shape == val.shape == (0,)


def test_topk_allocates_one_value_array_per_dtype_and_calls_under_the_lock(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: _FakeLib())
    t = _Thing(0)
    seen = []

    def call(idx_p, v32_p, v64_p, secs_p):
        seen.append(t._lock.locked())
        np.ctypeslib.as_array(C.cast(idx_p, C.POINTER(C.c_int64)), shape=(6,))[:] = np.arange(6)
        np.ctypeslib.as_array(C.cast(v32_p, C.POINTER(C.c_float)), shape=(6,))[:] = 0.5
        np.ctypeslib.as_array(C.cast(v64_p, C.POINTER(C.c_double)), shape=(6,))[:] = 0.25
        secs_p._obj.value = 2.0
        return 0

    idx, v32, v64, secs = t._topk(2, 3, (np.float32, np.float64), call)
    assert seen == [True] and not t._lock.locked() and secs == 2.0
    assert idx.dtype == np.int64 and idx.tolist() == [[0, 1, 2], [3, 4, 5]]
    assert v32.dtype == np.float32 and v64.dtype == np.float64 and v32.shape == v64.shape == (2, 3)
    assert (v32 == 0.5).all() and (v64 == 0.25).all()
    with pytest.raises(RuntimeError, match="error 1"):
        t._topk(0, 3, (np.int32,), lambda idx_p, v_p, secs_p: 1)
    assert not t._lock.locked()


def test_gallery_queries_checks_the_dimension():
    g = object.__new__(_lib.Gallery)
    g.d = 4
    a, code, rs, cs = g._queries(np.zeros((3, 8), np.float64)[:, ::2])
    assert a.shape == (3, 4) and (code, rs, cs) == (_lib.MI_F64, 8, 2)
    with pytest.raises(ValueError, match="^query dimension 5 != gallery dimension 4$"):
        g._queries(np.zeros((3, 5), np.float32))
    for name in ("search", "dense_search", "search_l2", "range_search", "rank_all", "refine"):
        with pytest.raises(ValueError, match="query dimension 5 != gallery dimension 4"):
            getattr(g, name)(np.zeros((3, 5), np.float32), *((1, 1) if name == "refine" else (1,)))


def test_search_refined_refuses_a_device_bitmap_first():
    with pytest.raises(ValueError, match="^refine takes allow, not allow_ptr$"):
        _lib._search_refined(object(), None, 1, 1, _lib._resolve_allow(None, 12345, 10, 0), 0, None, None)
    with pytest.raises(ValueError, match="refine must be a Gallery"):
        _lib._search_refined(object(), None, 1, 1, _lib._NO_ALLOW, 0, None, None)
