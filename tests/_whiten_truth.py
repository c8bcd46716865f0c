"""Shared helpers of the whitening GPU tests, pure numpy.

Scatter matrix (tests/test_gpu_whitenlearn.py, tests/test_gpu_input_layouts_proj.py): mi_scatter_matrix_device on torch tensors,
the float64 numpy scatter and the any-order bound |C_ij - ref_ij| <= 2 n u sqrt(C_ii C_jj), u = 2^-53 (Cauchy-Schwarz on the
standard dot-product error bound).

Whitening apply (tests/test_gpu_whiten_apply_reference.py, tests/test_whiten_truth_cpu.py): lattice problems on which
P[:dims] (x - m) is exact in float64 in any summation order (whiten_lattice_problem, beyond_float32, whiten_exact), the bit
comparison (check_bits), the derived bound of the normalised output (check_normalised), what a MI_NORM_NONE gallery must hold
(whiten_rows_f32), and the shapes both files walk."""
import math

import numpy as np

U = 2.0 ** -53


def _torch():
    import torch
    return torch


class DevScatter:
    """mi_scatter_matrix_device on torch tensors."""

    def __init__(self, lib, d):
        torch = _torch()
        self.lib, self.d = lib, d
        self.ws_bytes = lib.scatter_workspace_bytes(d)
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device="cuda")

    def __call__(self, rows, centre=None, pairs=None, into=None):
        """rows: CUDA tensor view [n, d]; centre: numpy [d] | None; pairs: (q, p) numpy int64; into: accumulate onto it."""
        torch = _torch()
        n, d = rows.shape
        C = into if into is not None else torch.empty((d, d), dtype=torch.float64, device="cuda")
        c = None if centre is None else torch.from_numpy(np.ascontiguousarray(centre, dtype=np.float64)).cuda()
        q = p = None
        if pairs is not None:
            q = torch.from_numpy(np.ascontiguousarray(pairs[0], dtype=np.int64)).cuda()
            p = torch.from_numpy(np.ascontiguousarray(pairs[1], dtype=np.int64)).cuda()
        self.lib.scatter_matrix_device(rows.data_ptr(), n, d, C.data_ptr(), self.ws.data_ptr(), self.ws_bytes,
                                       None if c is None else c.data_ptr(), None if q is None else q.data_ptr(),
                                       None if p is None else p.data_ptr(), 0 if q is None else q.numel(),
                                       into is not None, self.lib.MI_F32 if rows.dtype == torch.float32 else self.lib.MI_F64,
                                       rows.stride(0), rows.stride(1), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return C


def _check(C, ref, n, what):
    """Asserts the any-order bound, exact symmetry; returns the largest observed ratio error / bound."""
    assert np.array_equal(C, C.T), what + ": C != C.T"
    dg = np.sqrt(np.abs(np.diag(ref)))
    bound = 2.0 * n * U * np.outer(dg, dg)
    err = np.abs(C - ref)
    ok = err <= bound
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
    assert ok.all(), "%s: %d entries beyond 2 n u sqrt(C_ii C_jj), largest ratio %.3f" % (what, int((~ok).sum()), ratio)
    return ratio


def _ref_scatter(x, centre):
    xc = x.astype(np.float64) - (0.0 if centre is None else centre[None, :])
    return xc.T @ xc


# ---- whitening apply: exact lattice problems ------------------------------------------------------------------------------
W_TILE, W_KC, APPEND_CHUNK = 128, 16, 32768      # csrc/whiten.hip: outputs per workgroup, K chunk; csrc/api_gallery.hip: rows per turn
GRID_M = 2.0 ** -6                               # grid of m, of P and of float32 x - m
GRID_BEYOND = 2.0 ** -27                         # offset of beyond_float32: not a float32 beside 1 .. 3
GRID_Y = 2.0 ** -33                              # every exact output is a multiple of GRID_BEYOND * GRID_M

# (n, d, dims) of the product test, the smallest that reach each edge of whiten_mfma_kernel
PRODUCT_SHAPES = [
    (1, 1, 1), (1, 37, 37), (127, 15, 15), (128, 16, 16), (129, 17, 9),   # one tile; K below, at, beyond one chunk; n = 1
    (300, 130, 130), (257, 200, 129),                                    # 2 column tiles, plain order, ragged everywhere
    (300, 1000, 1000),                                                   # 8 column tiles: XCD order, ragged column / row / K
    (129, 1024, 1024), (128, 1030, 1024),                                # 8 full column tiles: fast on all chunks / off on the last
    (260, 1040, 1025),                                                   # 9 column tiles: the plain order again
    (130, 2000, 1930),                                                   # 16 column tiles: two column blocks per XCD
    (130, 1024, 900), (130, 1024, 896),                                  # 8 against 7 tiles from the same P
]
SAME_P = {(130, 1024, 896): 900}                 # this shape applies the first rows of the P of (n, d, 900)
# the last width of each normalisation kernel and the first of the next
NORM_SHAPES = [(129, 17, 9), (300, 1000, 1000), (5, 2048, 2048), (5, 2049, 2049), (5, 4096, 4096), (5, 4097, 4097)]
APPEND_FIRST, APPEND_SECOND, APPEND_D, APPEND_DIMS = 100, APPEND_CHUNK + 129, 20, 8
APPEND_SHAPE = (APPEND_FIRST + APPEND_SECOND, APPEND_D, APPEND_DIMS)
APPEND_EDGE = APPEND_FIRST + APPEND_CHUNK        # first gallery row the second turn of the append loop writes
APPEND_QUERY_ROWS = [APPEND_EDGE + o for o in (-8, -5, -3, -2, -1, 0, 1, 2, 6, 12)]     # ten rows on both sides of it
APPEND_ZERO_ROW = APPEND_EDGE + 3                # a second zero row, in the second turn (see append_where)


def _grid64(rng, shape):
    v = np.round(rng.standard_normal(shape) * 64.0) / 64.0
    v[v == 0] = 0.25
    return v


def _assert_exact(x64, m, P, grid_x):
    """The exactness precondition, on the numbers themselves: x - m lies on grid_x, P on GRID_M, and for every output
    sum_k |P_jk (x_k - m_k)| / (grid_x GRID_M) < 2^53.  Then every product and every partial sum of P (x - m), in ANY order
    (the one inside v_mfma_f64_16x16x4_f64 included), is an integer multiple of the grid below 2^53: no operation rounds."""
    xc = x64 - m[None, :]
    assert np.array_equal(np.rint(xc / grid_x) * grid_x, xc), "x - m is not on the 2^%d grid" % int(np.log2(grid_x))
    assert np.array_equal(np.rint(P / GRID_M) * GRID_M, P), "P is not on the 2^-6 grid"
    worst = float((np.abs(xc) @ np.abs(P).T).max()) / (grid_x * GRID_M)
    assert worst < 2.0 ** 53, "sum_k |P_jk (x_k - m_k)| / grid = 2^%.1f: the product is not exact" % np.log2(worst)
    return worst


def whiten_lattice_problem(n, d, dims, seed, zero_rows=()):
    """-> (x32 float32 [n, d], m float64 [d], P float64 [dims, d]) with P (x - m) exact in float64 in any summation order.

    x is integers in +-{1, 2, 3}; m and P are round(64 standard_normal) / 64 with zeros replaced by 1/4: every product is a
    multiple of 2^-12 and sum_k |P_jk| |x_k - m_k| stays far below 2^18, which _assert_exact checks on the numbers made.  P comes
    from a generator of its own, row after row, so the P of a smaller dims is the first rows of the P of a larger one
    (before the planting).

    Planted, for n >= 3 (a smaller problem would consist of nothing else):
      row 0 = m (on the 2^-6 grid below 8, so a float32): the centred row and its whole output row are exactly zero;
      row 1 = m except coordinate k0 = d // 2, where it is m + 2, and column k0 of P is zero except in row j0 = dims - 1:
      exactly one output column of row 1, the last, is not zero (2 P[j0, k0]);
      rows zero_rows = m as well."""
    assert n >= 1 and 1 <= dims <= d
    rx, rm, rp = (np.random.default_rng([seed, n, d, i]) for i in range(3))
    x = (rx.integers(1, 4, size=(n, d)) * rx.choice([-1, 1], size=(n, d))).astype(np.float32)
    m = _grid64(rm, (d,))
    P = _grid64(rp, (dims, d))
    if n >= 3:
        k0, j0 = d // 2, dims - 1
        keep = P[j0, k0]
        P[:, k0] = 0.0
        P[j0, k0] = keep
        x[0] = m.astype(np.float32)
        x[1] = x[0]
        x[1, k0] += np.float32(2.0)
        for r in zero_rows:
            x[r] = x[0]
        assert np.array_equal(x[0].astype(np.float64), m) and float(x[1, k0]) == m[k0] + 2.0
    _assert_exact(x.astype(np.float64), m, P, GRID_M)
    if n >= 3:
        y01 = whiten_exact(x[:2], m, P, dims)
        assert not y01[0].any() and np.flatnonzero(y01[1]).tolist() == [dims - 1]
    return x, m, P


def whiten_exact(x, m, P, dims):
    """float64 [n, dims] = (x - m) P[:dims]^T, the plain numpy product; x float32 or float64.  Exact by the precondition that
    whiten_lattice_problem / beyond_float32 asserted: whatever order the BLAS sums in, no operation rounds."""
    return (np.asarray(x, dtype=np.float64) - np.asarray(m, dtype=np.float64).reshape(1, -1)) @ np.asarray(P)[:dims].T


def beyond_where(n, d):
    """Elements beyond_float32 moves: the last row's last coordinate (ragged row tile, ragged K chunk) and a middle row's first;
    never the planted rows 0 and 1 of a problem with n >= 3."""
    return sorted({(n - 1, d - 1), (n // 2 if n < 3 else max(n // 2, 2), 0)})


def append_where():
    """beyond_where of the append problem and one element of each zero row: 2^-27 P[j, c] vanishes when an output of size 10
    is rounded to float32, so only a row that is zero without the offset shows in a gallery that float64 input was kept."""
    n, d, _ = APPEND_SHAPE
    return sorted(set(beyond_where(n, d)) | {(0, 0), (APPEND_ZERO_ROW, d - 1)})


def beyond_float32(x32, where, m, P):
    """float64 x = x32 with 2^-27 added at the (row, column) pairs of `where`: values float32 cannot hold beside 1 .. 3 and that
    round back to x32.  The products now lie on the 2^-33 grid; the exactness precondition is asserted again."""
    x64 = x32.astype(np.float64)
    for r, c in where:
        x64[r, c] += GRID_BEYOND
    assert np.array_equal(x64.astype(np.float32), x32) and int((x64 != x32).sum()) == len(where)
    _assert_exact(x64, m, P, GRID_BEYOND)
    return x64


def whiten_rows_f32(y_exact):
    """What a MI_NORM_NONE gallery must hold of exact whitened rows: each value rounded to float32 once, to nearest."""
    return np.asarray(y_exact, dtype=np.float64).astype(np.float32)


def check_bits(got, want, what):
    """dtype, shape and every bit of every value (array_equal on the values; the lattice outputs hold no NaN and no -0)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, "%s: %s %s, expected %s %s" % (what, got.dtype, got.shape, want.dtype, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        r, c = (int(v) for v in bad[0])
        raise AssertionError("%s: %d of %d values differ, first at (%d, %d): %r, expected %r" %
                             (what, len(bad), got.size, r, c, got[r, c], want[r, c]))


def normalised_reference(y_exact, eps):
    """-> (ref float64 [n, dims], zero bool [n]): ref = y / (sqrt(ss) + eps) with ss the EXACT sum of squares of the row -- Python
    integers on the grid 2^-66 of the squares -- rounded to float64 once; zero marks the rows with ss == 0 (ref there: +0 under
    eps > 0, numpy's 0 / 0 = NaN under eps == 0)."""
    y = np.asarray(y_exact, dtype=np.float64)
    yi = y / GRID_Y
    assert np.array_equal(yi, np.rint(yi)) and float(np.abs(yi).max()) < 2.0 ** 62, "outputs are not on the 2^-33 grid"
    yo = yi.astype(np.int64).astype(object)
    ss = [int(s) for s in (yo * yo).sum(axis=1)]
    nrm = np.array([math.sqrt(s) for s in ss], dtype=np.float64) * GRID_Y        # int -> float64 rounds once, to nearest
    with np.errstate(invalid="ignore", divide="ignore"):
        ref = y / (nrm + eps)[:, None]
    return ref, np.array([s == 0 for s in ss])


def normalised_bound(dims):
    return (dims / 2.0 + 8.0) * U


def check_normalised(got, y_exact, eps, what):
    """Asserts |got - ref| <= (dims / 2 + 8) u |ref|, u = 2^-53, with ref of normalised_reference; returns the largest observed
    ratio error / bound.

    Derivation.  The device squares dims values (one rounding each) and sums the non-negative squares in some order: relative
    error <= dims u on ss, so <= dims u / 2 on its root.  The root, the addition of eps and the division add at most 4 u between
    them (the root within one unit in the last place, 2 u; the other two correctly rounded, u each).  The reference's own
    roundings -- the exact ss to float64 (u, halved by the root), root, add, divide: 3.5 u -- are covered by the remaining 4 u.
    Terms of second order are below 2^-80 at dims <= 4097.  Nothing in the bound is measured on a device.

    A row with ss == 0 must be all +0.0 under eps > 0 and all NaN under eps == 0 (0 / 0, what the reference gives); every other
    row must be finite."""
    assert eps >= 0.0
    got, y = np.asarray(got), np.asarray(y_exact, dtype=np.float64)
    assert got.dtype == np.float64 and got.shape == y.shape, "%s: %s %s, expected float64 %s" % (what, got.dtype, got.shape, y.shape)
    ref, zero = normalised_reference(y, eps)
    for r in np.flatnonzero(zero):
        if eps > 0:
            assert not got[r].any() and not np.signbit(got[r]).any(), "%s: zero row %d is not all +0.0" % (what, r)
        else:
            assert np.isnan(got[r]).all(), "%s: zero row %d under eps = 0 is not all NaN" % (what, r)
    g, f = got[~zero], ref[~zero]
    assert np.isfinite(g).all(), "%s: %d values of non-zero rows are not finite" % (what, int((~np.isfinite(g)).sum()))
    err, bound = np.abs(g - f), normalised_bound(y.shape[1]) * np.abs(f)
    ok = err <= bound
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0)), initial=0.0))
    assert ok.all(), "%s: %d values beyond (dims / 2 + 8) u |ref|, largest ratio %.3g" % (what, int((~ok).sum()), ratio)
    return ratio


_problems = {}


def problem(n, d, dims, seed=20):
    """whiten_lattice_problem, made once per shape and shared read-only; a SAME_P shape gets the x, m and P of its partner."""
    key = (n, d, SAME_P.get((n, d, dims), dims), seed)
    if key not in _problems:
        _problems[key] = whiten_lattice_problem(*key, zero_rows=(APPEND_ZERO_ROW,) if (n, d, dims) == APPEND_SHAPE else ())
        for a in _problems[key]:
            a.setflags(write=False)
    return _problems[key]
