"""GPU: whitening apply (csrc/whiten.hip: whiten_mfma_kernel, rownorm_f64_kernel<8>, <16>, rownorm_f64_wide_kernel) and the chunk loop
of mi_gallery_append_whitened_device (csrc/api_gallery.hip) against an exact reference, at the shapes where their control flow
changes: tile, loader and chunk edges, both block orders, every normalisation kernel's last width and the next one's first, a
second turn of the 32 768-row append loop.

The product P[:dims] (x - m) is compared BIT FOR BIT: tests/_whiten_truth.py makes lattice problems on which every product and
every partial sum is exact in float64 in any order (the precondition is asserted on the numbers, on the CPU, in
tests/test_whiten_truth_cpu.py as well).  The normalised output is compared with the derived bound of check_normalised,
(dims / 2 + 8) u |ref| against a reference whose sum of squares is exact; nothing in it was measured on a device.  Largest
observed ratio to that bound on an MI355X: 0 (printed by test_normalised_output): on the lattice the sums of squares are exact in
float64 too, in all but the rows moved by 2^-27, and the device's root, sum and quotient are the reference's.

Every device output lies between two guard rows that hold a sentinel, as does every value of the output before the launch: a
value the kernel does not write, or writes outside its rows, fails the comparison."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _whiten_truth as wt  # noqa: E402

SENT = -7.25e300


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from isehr_amd import _lib
    _lib.load()
    return _lib


def _stream():
    return wt._torch().cuda.current_stream().cuda_stream


def _dev(a):
    return wt._torch().from_numpy(np.array(a, order="C")).cuda()      # (a copy: the shared problems are read-only)


class Source:
    """One layout of one [n, d] array: `host`, a numpy view for mi_whiten_apply, and the same bytes on the device with the
    element strides (rs, cs) for mi_whiten_apply_device; ptr_of_row(r) is the address of row r."""

    def __init__(self, lib, values, layout):
        torch = wt._torch()
        n, d = values.shape
        self.name, self.n, self.d = "%s %s" % (values.dtype.name, layout), n, d
        self.code, self.esz = (lib.MI_F32, 4) if values.dtype == np.float32 else (lib.MI_F64, 8)
        if layout == "rows":
            self.host, self.rs, self.cs, off = values, d, 1, 0
            self.t = _dev(values)
        elif layout == "DN":                                   # the reference's [D, N] array, seen as rows: rs = 1, cs = n
            dn = np.ascontiguousarray(values.T)
            self.host, self.rs, self.cs, off = dn.T, 1, n, 0
            self.t = _dev(dn)
        else:                                                  # every other column of a wider tensor whose other columns are NaN
            wide = np.full((n, 2 * d + 1), np.nan, values.dtype)
            wide[:, 1::2] = values
            self.host, self.rs, self.cs, off = wide[:, 1::2], 2 * d + 1, 2, 1
            self.t = _dev(wide)
        assert np.array_equal(self.host, values)
        self.ptr = self.t.data_ptr() + off * self.esz
        torch.cuda.synchronize()

    def ptr_of_row(self, r):
        return self.ptr + r * self.rs * self.esz


def _operands(shape):
    """(x32, x64 beyond float32, m, P) of a shape and (m, P) on the device, made once."""
    if shape not in _operands.cache:
        n, d, dims = shape
        x, m, P = wt.problem(n, d, dims)
        x64 = wt.beyond_float32(x, wt.append_where() if shape == wt.APPEND_SHAPE else wt.beyond_where(n, d), m, P)
        _operands.cache[shape] = (x, x64, m, P, _dev(m), _dev(P))
    return _operands.cache[shape]


_operands.cache = {}


def _apply_device(lib, src, md, Pd, dims, eps):
    """mi_whiten_apply_device into rows 1 .. n of a sentinel-filled [n + 2, dims] buffer; the guard rows must come back untouched."""
    torch = wt._torch()
    buf = torch.full((src.n + 2, dims), SENT, dtype=torch.float64, device="cuda")
    lib.whiten_apply_device(src.ptr, src.n, src.d, md.data_ptr(), Pd.data_ptr(), dims, buf[1:].data_ptr(), eps=eps, dtype=src.code,
                            row_stride=src.rs, col_stride=src.cs, stream=_stream())
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    assert (h[0] == SENT).all() and (h[-1] == SENT).all(), "%s: a guard row was written" % src.name
    return np.ascontiguousarray(h[1:-1])


# ---- a. the product, bit for bit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", wt.PRODUCT_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_product_bit_for_bit(lib, shape):
    n, d, dims = shape
    x, x64, m, P, md, Pd = _operands(shape)
    want = {np.dtype(np.float32): wt.whiten_exact(x, m, P, dims), np.dtype(np.float64): wt.whiten_exact(x64, m, P, dims)}
    got = {}
    for values, layout in ((x, "rows"), (x, "DN"), (x, "strided"), (x64, "rows"), (x64, "DN")):
        src = Source(lib, values, layout)
        what = "%d x %d -> %d, %s" % (n, d, dims, src.name)
        y = _apply_device(lib, src, md, Pd, dims, -1.0)
        wt.check_bits(y, want[values.dtype], what + ", mi_whiten_apply_device")
        wt.check_bits(_apply_device(lib, src, md, Pd, dims, -1.0), y, what + ", second call")
        wt.check_bits(lib.whiten_apply(src.host, m, P, dims, eps=-1.0), want[values.dtype], what + ", mi_whiten_apply")
        got[values.dtype, layout] = y
    for layout in ("rows", "DN"):
        assert not np.array_equal(got[np.dtype(np.float64), layout], got[np.dtype(np.float32), layout]), \
            "%d x %d -> %d, %s: float64 input gives the answer of the rounded input" % (n, d, dims, layout)


# ---- b. the normalised output, against the derived bound ------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [1e-6, 0.0], ids=["eps1e-6", "eps0"])
@pytest.mark.parametrize("shape", wt.NORM_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_normalised_output(lib, shape, eps):
    n, d, dims = shape
    x, x64, m, P, md, Pd = _operands(shape)
    worst = 0.0
    for values, layout in ((x, "rows"), (x64, "DN")):
        src = Source(lib, values, layout)
        y = wt.whiten_exact(values, m, P, dims)
        assert not y[0].any() and np.flatnonzero(y[1]).tolist() == [dims - 1]          # the planted rows are there
        what = "%d x %d -> %d, eps %g, %s" % (n, d, dims, eps, src.name)
        worst = max(worst, wt.check_normalised(_apply_device(lib, src, md, Pd, dims, eps), y, eps, what + ", device"))
        worst = max(worst, wt.check_normalised(lib.whiten_apply(src.host, m, P, dims, eps=eps), y, eps, what + ", host"))
    print("normalised %d x %d -> %d, eps %g: largest |got - ref| / ((dims / 2 + 8) u |ref|) = %.3g" % (n, d, dims, eps, worst))


def test_whitenapply_hip_through_the_same_check(lib):
    """whiten.whitenapply_hip: [D, N] in, [dims, N] out, `dimensions` absent (all rows of P) and given."""
    from isehr_amd import whiten
    shape = (300, 1000, 1000)
    x, x64, m, P, _, _ = _operands(shape)
    for values in (x, x64):
        X = np.ascontiguousarray(values.T)                   # [D, N]
        for dimensions in (None, 900):
            dims = 1000 if dimensions is None else dimensions
            out = whiten.whitenapply_hip(X, m.reshape(-1, 1), P) if dimensions is None else whiten.whitenapply_hip(X, m.reshape(-1, 1), P, dimensions)
            assert out.shape == (dims, 300)
            r = wt.check_normalised(np.ascontiguousarray(out.T), wt.whiten_exact(values, m, P, dims), 1e-6,
                                    "whitenapply_hip %s dimensions=%s" % (values.dtype.name, dimensions))
            print("whitenapply_hip %s dimensions=%s: ratio to the bound %.3g" % (values.dtype.name, dimensions, r))


# ---- c. the append across the chunk boundary ----------------------------------------------------------------------------------
def _append_both(lib, g, src, md, Pd):
    """rows [0, APPEND_FIRST) in one call, the rest -- one full turn of the chunk loop and 129 rows of a second -- in another"""
    for r0, k in ((0, wt.APPEND_FIRST), (wt.APPEND_FIRST, wt.APPEND_SECOND)):
        g.append_whitened_device(src.ptr_of_row(r0), k, src.d, md.data_ptr(), Pd.data_ptr(), dtype=src.code, row_stride=src.rs,
                                 col_stride=src.cs, stream=_stream())
    wt._torch().cuda.synchronize()


def _library_n(lib, g):
    n = C.c_int64()
    lib.check(lib.load().mi_gallery_info(g._h, C.byref(n), None, None, None, None, None))
    return n.value


def test_append_across_the_chunk_boundary(lib):
    n, d, dims = wt.APPEND_SHAPE
    x, x64, m, P, md, Pd = _operands(wt.APPEND_SHAPE)
    for values, layout in ((x, "rows"), (x64, "DN")):
        src = Source(lib, values, layout)
        want = wt.whiten_rows_f32(wt.whiten_exact(values, m, P, dims))
        with lib.Gallery.empty(n + 1, dims, norm_mode=lib.NORM_NONE) as g:
            _append_both(lib, g, src, md, Pd)
            assert g.n == n and _library_n(lib, g) == n
            wt.check_bits(g.get_rows(0, n), want, "append, %s" % src.name)
            # refusals: one row beyond the capacity; a gallery wider than d.  Neither changes n or a row.
            with pytest.raises(RuntimeError, match="capacity"):
                g.append_whitened_device(src.ptr_of_row(0), 2, d, md.data_ptr(), Pd.data_ptr(), dtype=src.code, row_stride=src.rs,
                                         col_stride=src.cs, stream=_stream())
            with pytest.raises(RuntimeError, match="bad sizes"):
                g.append_whitened_device(src.ptr_of_row(0), 1, dims - 1, md.data_ptr(), Pd.data_ptr(), dtype=src.code,
                                         row_stride=src.rs, col_stride=src.cs, stream=_stream())
            assert g.n == n and _library_n(lib, g) == n
            wt.check_bits(g.get_rows(0, n), want, "append, %s, after the refusals" % src.name)
    kept = wt.whiten_rows_f32(wt.whiten_exact(x64, m, P, dims))
    assert not np.array_equal(kept[wt.APPEND_ZERO_ROW], wt.whiten_rows_f32(wt.whiten_exact(x, m, P, dims))[wt.APPEND_ZERO_ROW])


def test_append_normalises_every_chunk(lib):
    """The same rows into a MI_NORM_L2_EPS gallery: rows 32 760 .. 32 780 of the second append within float32 rounding of the
    reference of check_normalised, and found by the search."""
    n, d, dims = wt.APPEND_SHAPE
    x, _, m, P, md, Pd = _operands(wt.APPEND_SHAPE)
    y = wt.whiten_exact(x, m, P, dims)
    lo, hi = wt.APPEND_FIRST + 32760, wt.APPEND_FIRST + 32781
    ref, zero = wt.normalised_reference(y[lo:hi], 1e-6)
    assert zero.sum() == 1 and lo < wt.APPEND_EDGE < hi
    with lib.Gallery.empty(n, dims, norm_mode=lib.NORM_L2_EPS) as g:
        _append_both(lib, g, Source(lib, x, "rows"), md, Pd)
        got = g.get_rows(lo, hi - lo).astype(np.float64)
        err = np.abs(got - ref)
        print("normalised append: largest |row - ref| / (2^-24 |ref|) = %.3f" % float(np.max(err[ref != 0] / (2.0 ** -24 * np.abs(ref[ref != 0])))))
        assert (err <= 2.0 ** -24 * np.abs(ref)).all()
        ids = np.array(wt.APPEND_QUERY_ROWS)
        idx, sc, _ = g.search(g.get_rows(0, n)[ids], 5)
        assert np.array_equal(idx[:, 0], ids), idx[:, 0]
        assert np.abs(sc[:, 0] - 1.0).max() < 1e-5


def test_append_into_an_l2_gallery(lib):
    """The squared-L2 gallery takes the same two appends (launch_l2_bias behind the chunk loop): ten rows from both sides of the
    boundary are their own first hit at distance 0, and every answer is that of a gallery made of the same float32 rows."""
    n, d, dims = wt.APPEND_SHAPE
    x, _, m, P, md, Pd = _operands(wt.APPEND_SHAPE)
    want = wt.whiten_rows_f32(wt.whiten_exact(x, m, P, dims))
    ids = np.array(wt.APPEND_QUERY_ROWS)
    app = lib.Gallery.l2_from_host(None, d=dims, capacity=n)
    try:
        _append_both(lib, app, Source(lib, x, "rows"), md, Pd)
        assert app.n == n
        wt.check_bits(app.get_rows(0, n), want, "append into an L2 gallery")
        one = lib.Gallery.l2_from_host(want)
        try:
            a, b = app.search_l2(want[ids], 5), one.search_l2(want[ids], 5)
            assert np.array_equal(a[0][:, 0], ids), a[0][:, 0]
            assert not a[2][:, 0].any() and (a[2][:, 1] > 0).all()
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[2].view(np.uint64), b[2].view(np.uint64))
            assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
        finally:
            one.close()
    finally:
        app.close()
