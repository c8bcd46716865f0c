"""Input layouts for the typed, strided entry points of include/mi355_retrieval.h (tests only, pure numpy).

layouts(a, poison) embeds the values of a C-contiguous float32 [n, d] array in larger buffers, one per layout, and yields the
views.  Every buffer element that is not part of its view holds `poison` (NaN, or 1e30 where the entry point refuses
non-finite input whole-buffer), so that a read outside the view changes the answer instead of passing silently.  The sweep of
tests/test_gpu_input_layouts*.py feeds each view to each entry point and compares every output, byte for byte, with the answer
for the contiguous float32 array.  typed_entry_points() and EXCLUDED are the guard of tests/test_layouts_cpu.py."""
import collections
import os
import re

import numpy as np

GUARD = 4                     # poison elements before and after the flat layouts (c, t, bcast)
SUB_ROW0, SUB_COL0 = 5, 3     # the corner of sub32 in its buffer
SUB_ROWS, SUB_COLS = 4, 6     # rows below and columns right of sub32

# one view: its name, the view, the buffer that owns it, the element strides the construction claims and the number of poison
# elements the construction leaves in the buffer
Layout = collections.namedtuple("Layout", "name view buf rs cs n_poison")

QUERY_ONLY = ("bcast32",)     # rs = 0: every row is row 0


def _poisoned(shape, dtype, poison):
    return np.full(shape, poison, dtype=dtype)


def layouts(a, poison=np.nan, bcast=False):
    """a: C-contiguous float32 [n, d] -> Layout tuples c32 c64 t32 t64 pad32 pad64 col32 col64 sub32 (and bcast32 with
    bcast=True, whose view holds row 0 of `a` n times)."""
    a = np.asarray(a)
    assert a.dtype == np.float32 and a.ndim == 2 and a.flags.c_contiguous and a.size > 0
    n, d = a.shape
    for bits, dt in ((32, np.float32), (64, np.float64)):
        flat = _poisoned(n * d + 2 * GUARD, dt, poison)
        v = flat[GUARD:GUARD + n * d].reshape(n, d)
        v[...] = a
        yield Layout("c%d" % bits, v, flat, d, 1, 2 * GUARD)
    for bits, dt in ((32, np.float32), (64, np.float64)):
        flat = _poisoned(n * d + 2 * GUARD, dt, poison)
        v = flat[GUARD:GUARD + n * d].reshape(d, n).T              # the reference's [D, N] arrays, seen as rows
        v[...] = a
        yield Layout("t%d" % bits, v, flat, 1, n, 2 * GUARD)
    for bits, dt in ((32, np.float32), (64, np.float64)):
        buf = _poisoned((n, d + 3), dt, poison)
        v = buf[:, :d]
        v[...] = a
        yield Layout("pad%d" % bits, v, buf, d + 3, 1, 3 * n)
    for bits, dt in ((32, np.float32), (64, np.float64)):
        buf = _poisoned((n, 2 * d + 2), dt, poison)
        v = buf[:, 1:2 * d + 1:2]
        v[...] = a
        yield Layout("col%d" % bits, v, buf, 2 * d + 2, 2, n * (d + 2))
    buf = _poisoned((SUB_ROW0 + n + SUB_ROWS, SUB_COL0 + d + SUB_COLS), np.float32, poison)
    v = buf[SUB_ROW0:SUB_ROW0 + n, SUB_COL0:SUB_COL0 + d]
    v[...] = a
    yield Layout("sub32", v, buf, SUB_COL0 + d + SUB_COLS, 1, buf.size - n * d)
    if bcast:
        flat = _poisoned(d + 2 * GUARD, np.float32, poison)
        flat[GUARD:GUARD + d] = a[0]
        v = np.broadcast_to(flat[GUARD:GUARD + d], (n, d))
        yield Layout("bcast32", v, flat, 0, 1, 2 * GUARD)


def expected(lay, a):
    """The values the view of `lay` holds, as a contiguous float32 array: `a`, for bcast32 row 0 of `a` n times."""
    return np.ascontiguousarray(np.broadcast_to(a[:1], a.shape)) if lay.name in QUERY_ONLY else a


def element_strides(v):
    return tuple(s // v.dtype.itemsize for s in v.strides)


def offset_elements(lay):
    """Position of element (0, 0) of the view in its buffer, in elements."""
    return (lay.view.__array_interface__["data"][0] - lay.buf.__array_interface__["data"][0]) // lay.buf.dtype.itemsize


def count_poison(lay, poison):
    b = lay.buf.ravel()
    return int(np.isnan(b).sum()) if np.isnan(poison) else int((b == poison).sum())


def on_device(lay):
    """The view of `lay` as a torch tensor on the GPU with the same element strides over a copy of the whole poisoned buffer."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(lay.buf).ravel()).cuda()
    return torch.as_strided(t, lay.view.shape, element_strides(lay.view), offset_elements(lay))


def beyond_float32(a, rows, cols):
    """a64 = float64(a) with 2^-30 |a| added to the planted elements (rows x cols): float64 values that float32 cannot hold and
    that round back to `a`."""
    a64 = a.astype(np.float64)
    for r in rows:
        for c in cols:
            assert a[r, c] != 0
            a64[r, c] += 2.0 ** -30 * abs(a64[r, c])
    assert np.array_equal(a64.astype(np.float32), a) and not np.array_equal(a64, a.astype(np.float64))
    return a64


def load_lib():
    """Builds (if needed) and loads the library: the body of every GPU file's module-scoped `lib` fixture."""
    import __graft_entry__
    __graft_entry__.build()
    from isehr_amd import _lib
    _lib.load()
    return _lib


def same(got, want, what):
    """Two tuples of arrays equal in dtype, shape and bytes; the first differing element is named."""
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, "%s: output %d is %s %s, expected %s %s" % (what, i, g.dtype, g.shape, w.dtype, w.shape)
        if g.tobytes() != w.tobytes():
            rows = g.view(np.uint8).reshape(g.size, -1) != w.view(np.uint8).reshape(w.size, -1)
            at = int(np.flatnonzero(rows.any(1))[0])
            raise AssertionError("%s: output %d differs, first at flat element %d: %r, expected %r" % (what, i, at, g.ravel()[at], w.ravel()[at]))


def differs(a, b):
    return any(np.asarray(x).tobytes() != np.asarray(y).tobytes() for x, y in zip(a, b))


# ---- the guard -------------------------------------------------------------------------------------------------------------
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mi355_retrieval.h")

# typed entry points the sweep leaves out, each with its reason
EXCLUDED = {
    "mi_kr_rerank": "two typed arrays (queries and gallery) share one dtype and carry strides of their own, so it is no row of a "
                    "one-argument sweep; its layouts and dtypes are swept by test_gpu_kr_rerank.py / test_gpu_kr_rerank_edges.py",
}


def typed_entry_points(path=HEADER):
    """Every function the header declares whose parameter list contains `int dtype`, in declaration order."""
    with open(path) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    names = []
    for m in re.finditer(r"\b(mi_\w+)\s*\(([^;{}()]*)\)\s*;", text):
        if re.search(r"\bint\s+dtype\b", m.group(2)):
            names.append(m.group(1))
    return names
