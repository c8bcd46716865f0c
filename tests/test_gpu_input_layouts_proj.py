"""GPU: the typed, strided entry points of the projection family (LSH encode, column sums, scatter matrix, whitening), fed each
layout of tests/_layouts.py from host memory (host forms) or from device memory (`*_device` forms).  Every output must equal,
byte for byte, the answer for the contiguous float32 array.

The rows are integer-lattice values, the directions, means and projections lie on a 2^-6 grid: every float64 product and every
partial sum is exact in any order, so the contiguous answer is compared with a float64 numpy product with == (an error of 0 is
inside the any-order bound 2 n u sqrt(C_ii C_jj) of test_gpu_whitenlearn.py).  The scatter matrix of float64 input that float32
cannot hold is not exact (its squares need more than 53 bits): there test_gpu_whitenlearn.py's own check and bound are used.

This family never rounds float64 to float32 ("x promoted to double"): float64 input that float32 cannot hold must give the
float64 numpy answer, and row 0 is planted so that this differs from the answer for the rounded input (an LSH projection that
equals its threshold until the offset lowers it; a whitened row that is exactly zero until the offset)."""
import numpy as np
import pytest

import _layouts as L
from _whiten_truth import DevScatter, _check, _ref_scatter

pytestmark = pytest.mark.gpu

N, NBITS = 600, 16
DS = [37, 130, 1]
SHAPES = [(N, 37), (N, 130), (N, 1), (1, 37)]


@pytest.fixture(scope="module")
def lib():
    return L.load_lib()


def _grid(rng, shape):
    v = np.round(rng.standard_normal(shape) * 64.0) / 64.0
    v[v == 0] = 0.25
    return v


class Problem:
    def __init__(self, d):
        rng = np.random.default_rng(d + 11)
        self.d, self.dims = d, min(d, 24)
        self.R = _grid(rng, (NBITS, d))
        self.R[0, 0] = -abs(self.R[0, 0])
        self.P = _grid(rng, (self.dims, d))
        self.centre = _grid(rng, (d,))

    def rows(self, n):
        x = np.random.default_rng(n + self.d).integers(1, 4, size=(n, self.d)).astype(np.float32)
        x *= np.random.default_rng(n).choice([-1.0, 1.0], size=x.shape).astype(np.float32)
        x[0, 0] = abs(x[0, 0])
        return x

    def operands(self, x):
        """thresholds and mean planted on row 0 of x: projection 0 equals its threshold, the centred row 0 is zero"""
        thr = np.full(NBITS, 0.5)
        thr[0] = float(x[0].astype(np.float64) @ self.R[0])
        return thr, x[0].astype(np.float64).copy()

    def pairs(self, n):
        rng = np.random.default_rng(n)
        return rng.integers(0, n, size=50).astype(np.int64), rng.integers(0, n, size=50).astype(np.int64)


def _dev(lib, x):
    import torch
    return x.data_ptr(), lib.MI_F32 if x.dtype == torch.float32 else lib.MI_F64, x.stride(0), x.stride(1)


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


# ---- calls: call(lib, p, x, x32) -> tuple of arrays; x a numpy view (host rows) or a device tensor (device rows); x32 the
# contiguous float32 values, from which the planted operands are made -------------------------------------------------------
def _lsh_host(lib, p, x, x32):
    return (lib.lsh_encode(x, p.R, p.operands(x32)[0]),)


def _lsh_device(lib, p, x, x32):
    import torch
    ptr, code, rs, cs = _dev(lib, x)
    R, thr = _t(p.R), _t(p.operands(x32)[0])
    out = torch.full((x.shape[0], NBITS // 8 + 3), 0xAA, dtype=torch.uint8, device="cuda")
    lib.lsh_encode_device(ptr, x.shape[0], p.d, R.data_ptr(), NBITS, out.data_ptr(), thr_ptr=thr.data_ptr(), dtype=code, row_stride=rs,
                          col_stride=cs, out_row_stride=NBITS // 8 + 3, stream=_stream())
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[:, NBITS // 8:] == 0xAA).all(), "bytes between the code rows were written"
    return (np.ascontiguousarray(o[:, :NBITS // 8]),)


def _lsh_append(lib, p, x, x32):
    import torch
    ptr, code, rs, cs = _dev(lib, x)
    R, thr = _t(p.R), _t(p.operands(x32)[0])
    n = x.shape[0]
    cut = n // 3
    with lib.BinaryGallery.empty(n, NBITS) as g:
        esz = 4 if code == lib.MI_F32 else 8
        for r0, m in ((0, cut), (cut, n - cut)):
            if m:
                g.append_lsh_device(ptr + r0 * rs * esz, m, p.d, R.data_ptr(), thr.data_ptr(), dtype=code, row_stride=rs, col_stride=cs,
                                    stream=_stream())
        torch.cuda.synchronize()
        return (g.get_codes(),)


def _lsh_truth(p, x, x32):
    proj = np.asarray(x, np.float64) @ p.R.T
    from isehr_amd import _lib
    return (_lib.pack_bits(proj >= p.operands(x32)[0][None, :]),)


def _colsum_device(lib, p, x, x32):
    import torch
    ptr, code, rs, cs = _dev(lib, x)
    out = torch.full((p.d,), -3.5e17, dtype=torch.float64, device="cuda")
    lib.column_sum_device(ptr, x.shape[0], p.d, out.data_ptr(), dtype=code, row_stride=rs, col_stride=cs, stream=_stream())
    torch.cuda.synchronize()
    return (out.cpu().numpy(),)


def _scatter_host(lib, p, x, x32):
    return (lib.scatter_matrix(x, centre=p.centre), lib.scatter_matrix(x, pairs=p.pairs(x.shape[0])))


def _scatter_device(lib, p, x, x32):
    dev = DevScatter(lib, p.d)
    return (dev(x, centre=p.centre).cpu().numpy(), dev(x, pairs=p.pairs(x.shape[0])).cpu().numpy())


def _scatter_truth(p, x, x32):
    x64 = np.asarray(x, np.float64)
    q, r = p.pairs(x.shape[0])
    diff = x64[q] - x64[r]
    return (_ref_scatter(x64, p.centre), diff.T @ diff)


def _whiten_host(lib, p, x, x32):
    return (lib.whiten_apply(x, p.operands(x32)[1], p.P, p.dims, eps=-1.0),)


def _whiten_device(lib, p, x, x32):
    import torch
    ptr, code, rs, cs = _dev(lib, x)
    m, P = _t(p.operands(x32)[1]), _t(p.P)
    out = torch.zeros((x.shape[0], p.dims), dtype=torch.float64, device="cuda")
    lib.whiten_apply_device(ptr, x.shape[0], p.d, m.data_ptr(), P.data_ptr(), p.dims, out.data_ptr(), eps=-1.0, dtype=code, row_stride=rs,
                            col_stride=cs, stream=_stream())
    torch.cuda.synchronize()
    return (out.cpu().numpy(),)


def _whiten_truth(p, x, x32):
    return ((np.asarray(x, np.float64) - p.operands(x32)[1][None, :]) @ p.P.T,)


def _whiten_append(lib, p, x, x32):
    import torch
    from _graph_truth import gallery_rows
    ptr, code, rs, cs = _dev(lib, x)
    m, P = _t(p.operands(x32)[1]), _t(p.P)
    n = x.shape[0]
    cut = n // 3
    esz = 4 if code == lib.MI_F32 else 8
    with lib.Gallery.empty(n, p.dims, norm_mode=lib.NORM_NONE) as g:
        for r0, k in ((0, cut), (cut, n - cut)):
            if k:
                g.append_whitened_device(ptr + r0 * rs * esz, k, p.d, m.data_ptr(), P.data_ptr(), dtype=code, row_stride=rs, col_stride=cs,
                                         stream=_stream())
        torch.cuda.synchronize()
        return (gallery_rows(g),)


# name -> (memory space of the swept argument, call, truth(p, x, x32) -> the tuple call must give)
ROWS = {
    "mi_lsh_encode": ("host", _lsh_host, _lsh_truth),
    "mi_lsh_encode_device": ("device", _lsh_device, _lsh_truth),
    "mi_hamming_append_lsh_device": ("device", _lsh_append, _lsh_truth),
    "mi_column_sum": ("host", lambda lib, p, x, x32: (lib.column_sum(x),), lambda p, x, x32: (np.asarray(x, np.float64).sum(0),)),
    "mi_column_sum_device": ("device", _colsum_device, lambda p, x, x32: (np.asarray(x, np.float64).sum(0),)),
    "mi_scatter_matrix": ("host", _scatter_host, _scatter_truth),
    "mi_scatter_matrix_device": ("device", _scatter_device, _scatter_truth),
    "mi_whiten_apply": ("host", _whiten_host, _whiten_truth),
    "mi_whiten_apply_device": ("device", _whiten_device, _whiten_truth),
    "mi_gallery_append_whitened_device": ("device", _whiten_append, lambda p, x, x32: (_whiten_truth(p, x, x32)[0].astype(np.float32),)),
}

_problems = {}


def _problem(d):
    if d not in _problems:
        _problems[d] = Problem(d)
    return _problems[d]


def _give(mem, lay_or_array):
    """the swept argument in the row's memory space: a numpy view as it stands, or its device twin"""
    import torch
    if mem == "host":
        return lay_or_array.view if isinstance(lay_or_array, L.Layout) else lay_or_array
    if isinstance(lay_or_array, L.Layout):
        t = L.on_device(lay_or_array)
    else:
        t = torch.from_numpy(np.ascontiguousarray(lay_or_array)).cuda()
    torch.cuda.synchronize()
    return t


@pytest.mark.parametrize("name", sorted(ROWS))
def test_layouts_give_the_contiguous_answer_and_the_truth(lib, name):
    mem, call, truth = ROWS[name]
    for n, d in SHAPES:
        p = _problem(d)
        a = p.rows(n)
        what = "%s, %d x %d" % (name, n, d)
        want = call(lib, p, _give(mem, a), a)
        L.same(want, truth(p, a, a), what + ", contiguous float32 against the float64 numpy product")
        for lay in L.layouts(a, np.nan):
            L.same(call(lib, p, _give(mem, lay), a), want, "%s, %s, %s" % (what, lay.name, mem))


@pytest.mark.parametrize("name", sorted(ROWS))
def test_float64_beyond_float32_is_kept(lib, name):
    mem, call, truth = ROWS[name]
    for d in DS:
        p = _problem(d)
        a = p.rows(N)
        a64 = L.beyond_float32(a, [0, 1, N - 1], [0])
        what = "%s, %d x %d, float64 beyond float32" % (name, N, d)
        got = call(lib, p, _give(mem, a64), a)
        want = truth(p, a64, a)
        if name.startswith("mi_scatter_matrix"):
            for C, ref in zip(got, want):
                _check(C, ref, N, what)                                  # the any-order bound 2 n u sqrt(C_ii C_jj)
        else:
            L.same(got, want, what)
        assert L.differs(got, call(lib, p, _give(mem, a), a)), what + ": the planted values do not tell the float64 answer from the rounded one"
        for lay in L.layouts(a, np.nan):
            if lay.name in ("t64", "col64"):
                lay.view[...] = a64
                L.same(call(lib, p, _give(mem, lay), a), got, what + ", " + lay.name)


def test_negative_strides_are_refused(lib):
    import ctypes as C
    p = _problem(37)
    a = p.rows(5)
    out = np.empty(37, np.float64)
    assert lib.load().mi_column_sum(C.c_void_p(a.ctypes.data), 5, 37, lib.MI_F32, -37, 1, 0, C.c_void_p(out.ctypes.data)) == lib.MI_ERR_INVALID
