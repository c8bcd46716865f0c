"""CPU: the truth and the checks of tests/test_gpu_whiten_apply_reference.py (tests/_whiten_truth.py) can fail.

Part one builds the lattice problem at every (n, d, dims) the GPU file uses -- that runs the exactness assertions of
whiten_lattice_problem and beyond_float32 where no device is needed -- and shows that an honest numpy model of the launch passes
every check.  Part two damages the model the ways whiten_mfma_kernel, the rownorm kernels and the chunk loop of
mi_gallery_append_whitened_device could be wrong; every damage must fail the check that guards it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _whiten_truth as wt  # noqa: E402

SENT = -7.25e300              # what an output buffer holds before the launch
ALL_SHAPES = sorted(set(wt.PRODUCT_SHAPES) | set(wt.NORM_SHAPES) | {wt.APPEND_SHAPE})


# ---- a numpy model of the launch -------------------------------------------------------------------------------------------
def block_tile(b, ncb, nrb, wrong=False):
    """(column tile, row tile) of workgroup b: csrc/whiten.hip; wrong = the XCD order with / and % exchanged."""
    if ncb % 8 == 0:
        x, j = b & 7, b >> 3
        return (x + 8 * (j % nrb), j // nrb) if wrong else (x + 8 * (j // nrb), j % nrb)
    return b % ncb, b // ncb


def model_product(x, m, P, dims, wrong_map=False, k_drop=False, k_clamp=False, skip_last_row=False, skip_last_cols=False,
                  swap_tiles=None):
    n, d = x.shape
    xc = np.asarray(x, np.float64) - m[None, :]
    kt = d - d % wt.W_KC
    Pm = P[:dims]
    if k_clamp:
        xc[:, kt:] = np.asarray(x, np.float64)[:, kt:] - m[d - 1]
    if k_drop:
        xc, Pm = xc[:, :kt], Pm[:, :kt]
    Y = xc @ Pm.T
    ncb, nrb = -(-dims // wt.W_TILE), -(-n // wt.W_TILE)
    out = np.full((n, dims), SENT)
    for b in range(ncb * nrb):
        cb, rt = block_tile(b, ncb, nrb, wrong_map)
        r0, c0 = rt * wt.W_TILE, cb * wt.W_TILE
        if r0 < n and c0 < dims:
            out[r0:r0 + wt.W_TILE, c0:c0 + wt.W_TILE] = Y[r0:r0 + wt.W_TILE, c0:c0 + wt.W_TILE]
    if swap_tiles:
        rt, ca, cb = swap_tiles
        rows = slice(rt * wt.W_TILE, (rt + 1) * wt.W_TILE)
        a, b = out[rows, ca * 128:ca * 128 + 128].copy(), out[rows, cb * 128:cb * 128 + 128].copy()
        out[rows, ca * 128:ca * 128 + 128], out[rows, cb * 128:cb * 128 + 128] = b, a
    if skip_last_row:
        out[n - 1] = SENT
    if skip_last_cols:
        out[:, dims - dims % wt.W_TILE:] = SENT
    return out


def model_norm(y, eps, drop_col=None, rows=None, no_eps=False, eps_inside=False):
    ss = (y * y).sum(axis=1)
    if drop_col is not None:
        sel = slice(None) if rows is None else rows
        ss[sel] = ss[sel] - y[sel, drop_col] ** 2
    with np.errstate(invalid="ignore", divide="ignore"):
        if no_eps:
            return y / np.sqrt(ss)[:, None]
        if eps_inside:
            return y / np.sqrt(ss + eps)[:, None]
        return y / (np.sqrt(ss) + eps)[:, None]


def model_append(x, m, P, dims, first, late=False, at_n=False):
    """Two appends (first rows, then the rest) through the chunk loop of mi_gallery_append_whitened_device into a MI_NORM_NONE
    gallery; late: the turns after the first read one row late; at_n: they ingest at g->n instead of g->n + r0."""
    n = x.shape[0]
    stored = np.full((n, dims), np.float32(-7.25e30), np.float32)
    gn = 0
    for s0, cnt in ((0, first), (first, n - first)):
        for r0 in range(0, cnt, wt.APPEND_CHUNK):
            rows = min(wt.APPEND_CHUNK, cnt - r0)
            src = np.minimum(np.arange(rows) + s0 + r0 + (1 if late and r0 else 0), n - 1)
            dst = gn + (0 if at_n and r0 else r0)
            stored[dst:dst + rows] = wt.whiten_rows_f32(wt.whiten_exact(x[src], m, P, dims))
        gn += cnt
    return stored


# ---- part one: the problems exist, are exact, and an honest model passes ---------------------------------------------------
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_problem_is_exact_and_the_model_passes(shape):
    n, d, dims = shape
    x, m, P = wt.problem(n, d, dims)                       # asserts the exactness precondition on the numbers it made
    assert x.dtype == np.float32 and x.shape == (n, d) and m.shape == (d,) and P.shape[1] == d and P.shape[0] >= dims
    y = wt.whiten_exact(x, m, P, dims)
    assert y.dtype == np.float64 and y.shape == (n, dims)
    assert np.array_equal(y / wt.GRID_Y, np.rint(y / wt.GRID_Y))
    if n >= 3:
        assert not y[0].any()
        assert np.flatnonzero(y[1]).tolist() == ([dims - 1] if P.shape[0] == dims else [])
        assert np.count_nonzero(y[2:]) > 0.99 * y[2:].size
    wt.check_bits(model_product(x, m, P, dims), y, "model")
    # another summation order gives the same bits: that is what exact means
    rev = (x.astype(np.float64) - m[None, :])[:, ::-1] @ P[:dims, ::-1].T
    wt.check_bits(rev, y, "reversed K order")
    x64 = wt.beyond_float32(x, wt.beyond_where(n, d), m, P)
    y64 = wt.whiten_exact(x64, m, P, dims)
    assert not np.array_equal(y64, y)
    wt.check_bits(model_product(x64, m, P, dims), y64, "model, float64 beyond float32")
    assert np.array_equal(wt.whiten_rows_f32(y), y.astype(np.float32))


@pytest.mark.parametrize("eps", [1e-6, 0.0])
@pytest.mark.parametrize("shape", wt.NORM_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_an_honest_float64_normalisation_is_inside_the_bound(shape, eps):
    n, d, dims = shape
    x, m, P = wt.problem(n, d, dims)
    for src in (x, wt.beyond_float32(x, wt.beyond_where(n, d), m, P)):
        y = wt.whiten_exact(src, m, P, dims)
        r = wt.check_normalised(model_norm(y, eps), y, eps, "numpy pairwise sum")
        # the plain left-to-right sum, the order furthest from the exact one
        ss = np.zeros(n)
        for c in range(dims):
            ss = ss + y[:, c] * y[:, c]
        with np.errstate(invalid="ignore", divide="ignore"):
            r2 = wt.check_normalised(y / (np.sqrt(ss) + eps)[:, None], y, eps, "sequential sum")
        assert max(r, r2) <= 1.0
        ref, zero = wt.normalised_reference(y, eps)
        assert zero.tolist() == [True] + [False] * (n - 1)
        assert np.isnan(ref[0]).all() if eps == 0 else not ref[0].any()


def test_append_rows_are_their_own_nearest():
    """The ten rows the GPU test searches for are alone at distance 0 (float32 rows) and at cosine 1 (normalised rows)."""
    n, d, dims = wt.APPEND_SHAPE
    x, m, P = wt.problem(n, d, dims)
    y = wt.whiten_exact(x, m, P, dims)
    rows = wt.whiten_rows_f32(y).astype(np.float64)
    ref, _ = wt.normalised_reference(y, 1e-6)
    assert min(wt.APPEND_QUERY_ROWS) < wt.APPEND_EDGE <= max(wt.APPEND_QUERY_ROWS) < n
    for r in wt.APPEND_QUERY_ROWS:
        d2 = ((rows - rows[r]) ** 2).sum(axis=1)
        d2[r] = np.inf
        assert d2.min() > 0
        cos = ref @ ref[r]
        own = cos[r]
        cos[r] = -np.inf
        assert own - cos.max() > 1e-4


# ---- part two: every damage fails its check ---------------------------------------------------------------------------------
def _fails(check, *args):
    with pytest.raises(AssertionError):
        check(*args)


def test_product_damages_fail_bit_equality():
    x, m, P = wt.problem(300, 1000, 1000)
    y = wt.whiten_exact(x, m, P, 1000)
    wt.check_bits(model_product(x, m, P, 1000), y, "undamaged")
    _fails(wt.check_bits, model_product(x, m, P, 1000, wrong_map=True), y, "cb = x + 8 (j % nrb)")
    _fails(wt.check_bits, model_product(x, m, P, 1000, swap_tiles=(1, 2, 5)), y, "two column tiles of row tile 1 exchanged")
    _fails(wt.check_bits, model_product(x, m, P, 1000, skip_last_row=True), y, "row n - 1 unwritten")
    _fails(wt.check_bits, model_product(x, m, P, 1000, skip_last_cols=True), y, "last dims % 128 columns unwritten")
    for n, d, dims in ((300, 1000, 1000), (128, 1030, 1024), (129, 17, 9), (1, 37, 37)):
        x, m, P = wt.problem(n, d, dims)
        y = wt.whiten_exact(x, m, P, dims)
        _fails(wt.check_bits, model_product(x, m, P, dims, k_drop=True), y, "last d % 16 columns of K dropped")
        if d % wt.W_KC > 1:                                  # (a tail of one column is column d - 1: its own mean)
            _fails(wt.check_bits, model_product(x, m, P, dims, k_clamp=True), y, "last d % 16 columns centred with m[d - 1]")
    # two column blocks per XCD, two row tiles: exchanging / and % is still a bijection of the tiles there, so the smallest
    # shape that tells the two mappings apart is one with nrb that does not divide into the column blocks: (300, 1000, 1000)
    x, m, P = wt.problem(130, 2000, 1930)
    wt.check_bits(model_product(x, m, P, 1930, wrong_map=True), wt.whiten_exact(x, m, P, 1930), "a bijection")


@pytest.mark.parametrize("shape", [(129, 17, 9), (300, 1000, 1000), (130, 2000, 1930)], ids=lambda s: "%dx%dx%d" % s)
def test_rounding_float64_input_fails_bit_equality(shape):
    n, d, dims = shape
    x, m, P = wt.problem(n, d, dims)
    x64 = wt.beyond_float32(x, wt.beyond_where(n, d), m, P)
    y64 = wt.whiten_exact(x64, m, P, dims)
    _fails(wt.check_bits, model_product(x64.astype(np.float32), m, P, dims), y64, "float64 input rounded to float32 first")
    # and through the float32 rows of a gallery, where the offset survives the rounding of the output in the zero rows only
    n, d, dims = wt.APPEND_SHAPE
    x, m, P = wt.problem(n, d, dims)
    x64 = wt.beyond_float32(x, wt.append_where(), m, P)
    kept, rounded = wt.whiten_rows_f32(wt.whiten_exact(x64, m, P, dims)), wt.whiten_rows_f32(wt.whiten_exact(x, m, P, dims))
    _fails(wt.check_bits, rounded, kept, "float64 input rounded to float32 first, seen through float32 rows")
    assert np.flatnonzero((kept != rounded).any(axis=1)).tolist() == [0, wt.APPEND_ZERO_ROW]      # one row in each turn of the loop


@pytest.mark.parametrize("shape", [(129, 17, 9), (300, 1000, 1000), (5, 4097, 4097)], ids=lambda s: "%dx%dx%d" % s)
def test_normalisation_damages_fail_the_bound(shape):
    n, d, dims = shape
    x, m, P = wt.problem(n, d, dims)
    y = wt.whiten_exact(x, m, P, dims)
    eps = 1e-6
    wt.check_normalised(model_norm(y, eps), y, eps, "undamaged")
    _fails(wt.check_normalised, model_norm(y, eps, drop_col=dims - 1), y, eps, "last column left out of every norm")
    _fails(wt.check_normalised, model_norm(y, eps, drop_col=dims - 1, rows=[1]), y, eps, "the one-column row's column left out")
    big = int(np.argmax(np.abs(y[2])))
    _fails(wt.check_normalised, model_norm(y, eps, drop_col=big, rows=[2]), y, eps, "one column left out of one ordinary row")
    _fails(wt.check_normalised, model_norm(y, eps, no_eps=True), y, eps, "eps left out")
    _fails(wt.check_normalised, model_norm(y[1:], eps, no_eps=True), y[1:], eps, "eps left out, no zero row to give it away")
    _fails(wt.check_normalised, model_norm(y, eps, eps_inside=True), y, eps, "eps inside the root")
    # the conventions of the zero row
    good0 = model_norm(y, 0.0)
    wt.check_normalised(good0, y, 0.0, "eps = 0")
    bad = good0.copy()
    bad[0] = 0.0
    _fails(wt.check_normalised, bad, y, 0.0, "zero row written as zeros under eps = 0")
    bad = model_norm(y, eps)
    bad[0] = np.nan
    _fails(wt.check_normalised, bad, y, eps, "zero row NaN under eps > 0")
    bad = model_norm(y, eps)
    bad[0, 0] = -0.0
    _fails(wt.check_normalised, bad, y, eps, "-0.0 in the zero row")
    bad = model_norm(y, eps)
    bad[2, 0] = np.nextafter(bad[2, 0], np.inf) * (1 + 4 * wt.normalised_bound(dims))
    _fails(wt.check_normalised, bad, y, eps, "one value four bounds away")


def test_append_damages_fail_bit_equality():
    n, d, dims = wt.APPEND_SHAPE
    x, m, P = wt.problem(n, d, dims)
    want = wt.whiten_rows_f32(wt.whiten_exact(x, m, P, dims))
    wt.check_bits(model_append(x, m, P, dims, wt.APPEND_FIRST), want, "undamaged")
    _fails(wt.check_bits, model_append(x, m, P, dims, wt.APPEND_FIRST, late=True), want, "second chunk read one row late")
    _fails(wt.check_bits, model_append(x, m, P, dims, wt.APPEND_FIRST, at_n=True), want, "second chunk ingested at g->n")
    # both show in the rows on either side of the boundary, which the GPU test also looks at through the normalised gallery
    for damaged in (model_append(x, m, P, dims, wt.APPEND_FIRST, late=True), model_append(x, m, P, dims, wt.APPEND_FIRST, at_n=True)):
        assert np.array_equal(damaged[:wt.APPEND_FIRST], want[:wt.APPEND_FIRST])
        assert not np.array_equal(damaged[wt.APPEND_EDGE:wt.APPEND_EDGE + 8], want[wt.APPEND_EDGE:wt.APPEND_EDGE + 8])
