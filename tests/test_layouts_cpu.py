"""CPU: the input layouts of tests/_layouts.py are what they claim to be, the binding passes them through without a copy, and
every typed entry point of include/mi355_retrieval.h is a row of the layout sweep (or excluded with a reason)."""
import importlib

import numpy as np
import pytest

import _layouts as L
from isehr_amd import _lib

SHAPES = [(7, 5), (70, 37), (1, 37), (1, 1), (70, 1), (3, 130)]
SWEEP_MODULES = ["test_gpu_input_layouts", "test_gpu_input_layouts_pq", "test_gpu_input_layouts_proj"]


def _a(n, d):
    return (np.arange(n * d, dtype=np.float32).reshape(n, d) + 1.0) * 0.5


def _claims(n, d):
    """name -> (dtype, row stride, col stride, poison count) as the issue's table states them"""
    out = {}
    for bits, dt in ((32, np.float32), (64, np.float64)):
        out["c%d" % bits] = (dt, d, 1, 2 * L.GUARD)
        out["t%d" % bits] = (dt, 1, n, 2 * L.GUARD)
        out["pad%d" % bits] = (dt, d + 3, 1, 3 * n)
        out["col%d" % bits] = (dt, 2 * d + 2, 2, n * (2 * d + 2) - n * d)
    out["sub32"] = (np.float32, d + L.SUB_COL0 + L.SUB_COLS, 1, (n + L.SUB_ROW0 + L.SUB_ROWS) * (d + L.SUB_COL0 + L.SUB_COLS) - n * d)
    out["bcast32"] = (np.float32, 0, 1, 2 * L.GUARD)
    return out


@pytest.mark.parametrize("n,d", SHAPES)
@pytest.mark.parametrize("poison", [np.nan, 1e30])
def test_layouts_are_what_they_claim(n, d, poison):
    a = _a(n, d)
    claims = _claims(n, d)
    seen = []
    for lay in L.layouts(a, poison, bcast=True):
        dt, rs, cs, n_poison = claims[lay.name]
        seen.append(lay.name)
        v = lay.view
        assert v.shape == (n, d) and v.dtype == dt and (lay.rs, lay.cs, lay.n_poison) == (rs, cs, n_poison)
        want = L.expected(lay, a)
        assert np.array_equal(v, want) and np.array_equal(v.astype(np.float32), want)
        # the element strides claimed; numpy is free in the stride of an axis of length 1, and the library never multiplies it
        got = L.element_strides(v)
        assert all(s * v.dtype.itemsize == b for s, b in zip(got, v.strides))
        if n > 1:
            assert got[0] == rs, (lay.name, got)
        if d > 1:
            assert got[1] == cs, (lay.name, got)
        # the view lies inside its buffer, and everything else in the buffer is poison
        off = L.offset_elements(lay)
        last = off + (n - 1) * got[0] + (d - 1) * got[1]
        assert 0 <= off and last < lay.buf.size
        assert L.count_poison(lay, poison) == n_poison
        assert lay.buf.size - n_poison == (d if lay.name == "bcast32" else n * d)
        # the binding hands the view itself to the library
        b, code, brs, bcs = _lib._strided(v)
        assert b.ctypes.data == v.ctypes.data and np.shares_memory(b, lay.buf)
        assert code == (_lib.MI_F32 if dt == np.float32 else _lib.MI_F64) and (brs, bcs) == got
    assert seen == ["c32", "c64", "t32", "t64", "pad32", "pad64", "col32", "col64", "sub32", "bcast32"]
    assert [lay.name for lay in L.layouts(a, poison)] == seen[:-1]


def test_unit_dimension_slices_keep_the_parent_strides():
    """(1, d) and (n, 1) slices report whatever strides their parent had: pad and col views of one row or one column"""
    for lay in L.layouts(_a(1, 37), np.nan):
        if lay.name in ("pad32", "col32", "sub32"):
            assert L.element_strides(lay.view)[0] == lay.rs
    for lay in L.layouts(_a(70, 1), np.nan):
        if lay.name in ("col32", "col64"):
            assert L.element_strides(lay.view) == (4, 2)


def test_only_negative_and_fractional_strides_are_copied():
    a = _a(6, 4)
    for v in (a[::-1], a[:, ::-1], a[::-2, ::-1]):
        b, code, rs, cs = _lib._strided(v)
        assert not np.shares_memory(b, a) and (rs, cs) == (4, 1) and np.array_equal(b, v)
    raw = np.zeros(6 * 18 + 16, np.uint8)
    odd = np.ndarray((6, 4), np.float32, buffer=raw, offset=0, strides=(18, 4))          # 18 bytes: no element multiple
    b, code, rs, cs = _lib._strided(odd)
    assert not np.shares_memory(b, raw) and (rs, cs) == (4, 1)
    for v in (a, a.T, a[::2], a[:, ::3], a[1:, 1:], np.broadcast_to(a[:1], (6, 4)), a.astype(np.float64)[:, 1:3]):
        b, code, rs, cs = _lib._strided(v)
        assert b.ctypes.data == v.ctypes.data and (rs, cs) == L.element_strides(v)


def test_beyond_float32_rounds_back():
    a = _a(5, 3)
    a64 = L.beyond_float32(a, [0, 4], [0, 2])
    assert (a64 != a).sum() == 4 and np.array_equal(a64.astype(np.float32), a)


def test_every_typed_entry_point_is_swept_or_excluded():
    names = L.typed_entry_points()
    assert len(names) == len(set(names)) >= 41 and "mi_graph_search" in names and "mi_pqw_train" in names
    swept = set()
    for mod in SWEEP_MODULES:
        swept |= set(importlib.import_module(mod).ROWS)
    assert not swept & set(L.EXCLUDED), "swept and excluded: %s" % sorted(swept & set(L.EXCLUDED))
    assert all(isinstance(r, str) and r for r in L.EXCLUDED.values())
    stale = sorted((swept | set(L.EXCLUDED)) - set(names))
    assert not stale, "not typed entry points of the header: %s" % stale
    missing = sorted(set(names) - swept - set(L.EXCLUDED))
    assert not missing, "typed entry points without a row in the layout sweep: %s" % missing
