"""CPU: the in-place update of the IVF-Flat index (mi_ivfflat_sync, mi_ivfflat_remove_rows) is declared, exported
and bound, answers a NULL handle and bad arguments through the loaded library before a handle is read, and IVFFlatIndex.remove
refuses a bad `rows` before it touches a handle.  What the calls compute is asserted on a real gallery in
tests/test_gpu_ivfflat_update.py."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"mi_ivfflat_sync": 2, "mi_ivfflat_remove_rows": 4}


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__
    __graft_entry__.build()
    from isehr_amd import _lib
    return _lib.load(), _lib


class _NoDevice:
    """Stands where a Gallery would: any use of its handle fails the test."""
    n, d, row_offset, device = 10, 4, 0, 0

    @property
    def _h(self):
        raise AssertionError("the handle was used")

    _lock = _h


def test_symbols_are_declared_exported_and_bound(built_lib):
    lib, _lib = built_lib
    hdr = open(os.path.join(ROOT, "include", "mi355_retrieval.h")).read()
    for name, nargs in NEW.items():
        assert "int %s(" % name in hdr, name
        assert hasattr(lib, name), name
        assert getattr(lib, name).restype == C.c_int
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
    assert "Not built: updating an index in place" not in hdr
    for meth in ("sync", "remove"):
        assert hasattr(_lib.IVFFlatIndex, meth), meth
    assert list(inspect.signature(_lib.IVFFlatIndex.sync).parameters) == ["self"]
    assert list(inspect.signature(_lib.IVFFlatIndex.remove).parameters) == ["self", "rows"]
    assert "sync()" in _lib.IVFFlatIndex.__doc__ and "remove()" in _lib.IVFFlatIndex.__doc__
    kernels = open(os.path.join(ROOT, "image-search-engine-for-historical-research_amd", "csrc", "kernels.h")).read()
    for launcher in ("launch_ivff_splice", "launch_ivff_compact"):
        assert "void %s(" % launcher in kernels, launcher


def test_invalid_arguments_answer_without_a_device(built_lib):
    lib, _lib = built_lib
    bits = np.zeros(1, np.uint64)
    out = C.c_int64(-7)
    P = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    fake = C.c_void_p(16)                         # non-null, never dereferenced: these checks answer before the handle is read
    assert lib.mi_ivfflat_sync(None, None) == _lib.MI_ERR_INVALID
    assert b"null handle" in lib.mi_last_error()
    assert lib.mi_ivfflat_sync(None, C.byref(out)) == _lib.MI_ERR_INVALID and out.value == -7
    for args, word in [((None, P(bits), _lib.MI_HOST, None), b"null handle"), ((None, None, _lib.MI_HOST, None), b"null handle"),
                       ((fake, None, _lib.MI_HOST, None), b"remove_bits"), ((fake, P(bits), 7, None), b"memspace"),
                       ((fake, P(bits), -1, C.byref(out)), b"memspace")]:
        assert lib.mi_ivfflat_remove_rows(*args) == _lib.MI_ERR_INVALID, args
        assert word in lib.mi_last_error(), (args, lib.mi_last_error())
    assert out.value == -7


def test_remove_raises_on_bad_rows_before_a_handle_is_read(built_lib):
    _, _lib = built_lib
    f = _lib.IVFFlatIndex.__new__(_lib.IVFFlatIndex)          # no handle at all: _h and _lock are never set
    f.gallery = _NoDevice()                                   # n = 10, row_offset = 0
    f.n = 10
    for rows in (np.array([10]), np.array([-1]), np.array([3, 11]), np.zeros(9, bool), np.zeros(11, bool), np.zeros((10, 1), bool),
                 np.zeros(10, np.float32), np.zeros(2, np.uint64).view(_lib.AllowBits)):
        with pytest.raises(ValueError):
            f.remove(rows)
    assert f.n == 10 and f.gallery.n == 10
