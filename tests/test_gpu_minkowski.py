"""GPU: exact Minkowski top-K on the raw rows (mi_knn_search_minkowski, mi_knn_search_minkowski_device, Gallery.search_minkowski,
KNN(..., 'l1' | 'linf' | 'lp'), matching_fractional_dis_hip(p=), MATCHING_METHODS['Lp']) against the numpy truth of
tests/_minkowski_truth.py.

"l1", "linf", "lp" with p == 1 and p == 2 must give the truth's ids and the truth's float64 BITS: the contract fixes the order of
every sum.  The data of those cases spans 48 binades, because sums of float32 values of one magnitude are exact in float64 and
would pass in any order.  p in {0.5, 1.5, 3} go against the high-accuracy reference (math.fsum of Python-float powers): the ids
must be the reference's, on inputs whose adjacent values lie at least 1e-9 apart (asserted on the reference alone), and the values
within 8 LP_MEASURED[p], eight times the largest deviation measured on an MI355X and never above 1e-10, a tenth of that gap."""
import numpy as np
import pytest

import _layouts as L
import _minkowski_truth as T

pytestmark = pytest.mark.gpu

QT = T.QT
EXACT = (("l1", None), ("linf", None), ("lp", 1), ("lp", 2))
# largest relative deviation of the device's values from the high-accuracy reference over the inputs of test_lp_against_reference,
# measured on an MI355X.  The tolerance of a p is 8 x its figure -- room for other inputs and another pow in a
# later ROCm -- and must stay at or below LP_CAP, a tenth of the gap the inputs guarantee, or the id comparison is not sound
LP_MEASURED = {0.5: 2.37e-16, 1.5: 2.52e-16, 3: 2.68e-16}
LP_CAP = 1e-10


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from isehr_amd import _lib
    _lib.load()
    return _lib


def _wide(seed, n, d):
    rng = np.random.default_rng([seed, n, d])
    return (rng.standard_normal((n, d)) * 2.0 ** rng.integers(-24, 24, (n, d))).astype(np.float32)


def _gauss(seed, n, d):
    return np.random.default_rng([seed, n, d]).standard_normal((n, d)).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(got, want):
    ids, dist, dist64 = got[:3]
    assert np.array_equal(ids, want[0])
    assert np.array_equal(_bits(dist64), _bits(want[1]))
    assert np.array_equal(dist, want[1].astype(np.float32))


def _check_exact(g, rows, q, k, allow=None, mask=None, off=0, metrics=EXACT):
    """every bit-exact metric of gallery g (whose stored rows are `rows`) against the truth; -> the answers by metric"""
    out = {}
    for metric, p in metrics:
        want = T.topk(T.values(rows, q, metric, p), k, allow=mask, row_offset=off)
        got = g.search_minkowski(q, k, metric, p, allow=allow)
        _same(got, want)
        out[(metric, p)] = got
    if ("l1", None) in out and ("lp", 1) in out:
        assert np.array_equal(_bits(out[("l1", None)][2]), _bits(out[("lp", 1)][2]))
    return out


def _device(g, q, k, metric, p, allow_words=None):
    import torch
    nq = q.shape[0]
    tq = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).cuda()
    idx = torch.full((nq, k), -7, dtype=torch.int64, device="cuda")
    d32 = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
    d64 = torch.zeros((nq, k), dtype=torch.float64, device="cuda")
    ta = None if allow_words is None else torch.from_numpy(np.ascontiguousarray(allow_words).view(np.int64)).cuda()
    torch.cuda.synchronize()
    g.search_minkowski_device(tq.data_ptr(), nq, k, idx.data_ptr(), metric, p, None if ta is None else ta.data_ptr(), d32.data_ptr(),
                              d64.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), d32.cpu().numpy(), d64.cpu().numpy()


# (n, d, nq, k): the float4 tail and the 256-column stride; the wave, scan-block and slab edges; the query-tile edges; k; and the
# narrower query tiles of wide rows (QT = 4, 2, 1 from d = 2561, 5121, 10241 on)
SHAPES = ([(65, d, QT + 1, 100) for d in (1, 3, 4, 255, 256, 257, 259, 2048)] +
          [(n, 20, 3, 100) for n in (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097)] +
          [(300, 37, nq, 1) for nq in (1, QT - 1, QT, QT + 1, 3 * QT + 2)] +
          [(4097, 5, 2, 2048), (2049, 6, 1, 2048), (1500, 7, 2, 2048), (2500, 9, 2, 1025)] +
          [(9, 2564, 5, 3), (9, 5124, 3, 3), (9, 10244, 2, 3)])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d-d%d-nq%d-k%d" % s)
def test_bit_exact_shapes(lib, shape):
    n, d, nq, k = shape
    rows, q = _wide(1, n, d), _wide(2, nq, d)
    with lib.Gallery.from_host(rows, norm_mode=lib.NORM_NONE) as g:
        _check_exact(g, rows, q, k)


def test_p2_is_the_l2_search_bit_for_bit(lib):
    """p == 2 on an L2 gallery: the ids and the float64 bits of Gallery.search_l2 (l2_direct_wave's walk), on data where the order
    of the sum shows.  Gallery.dense64_search_l2, the independent checker, sums in ANOTHER order (l2_dense_dist_kernel: 64 x 64
    tiles, columns in sequence), so on such data it differs from search_l2 itself in the last bits -- measured here on an MI355X:
    up to 11 ulp on these inputs -- and cannot equal this search bit for bit either: against it the ids must be equal and the values
    within the 2 d 2^-53 max-value bound under which tests/test_gpu_l2_search.py holds search_l2 to it.  Where every float64 sum is
    exact (integer rows: the squares and their sums stay below 2^53) all three must agree bit for bit."""
    n, d, nq, k = 3000, 259, QT + 3, 64
    rows, q = _wide(3, n, d), _wide(4, nq, d)
    with lib.Gallery.l2_from_host(rows) as g:
        ids, dist, dist64, _ = g.search_minkowski(q, k, "lp", 2)
        dense = g.dense64_search_l2(q, k)
        l2 = g.search_l2(q, k)
    assert np.array_equal(ids, l2[0]) and np.array_equal(_bits(dist64), _bits(l2[2])) and np.array_equal(dist, l2[1])
    ulps = np.abs(_bits(dist64).astype(np.int64) - _bits(dense[2]).astype(np.int64)).max()
    print("p = 2 against dense64_search_l2 on 48-binade data: %d ulp at the most; search_l2 against it: %d ulp"
          % (ulps, np.abs(_bits(l2[2]).astype(np.int64) - _bits(dense[2]).astype(np.int64)).max()))
    assert np.array_equal(ids, dense[0])
    assert (np.abs(dist64 - dense[2]) <= 2.0 * d * 2.0 ** -53 * dense[2].max(axis=1, keepdims=True)).all()
    rng = np.random.default_rng(5)
    rows, q = rng.integers(-8, 9, (n, d)).astype(np.float32), rng.integers(-8, 9, (nq, d)).astype(np.float32)
    with lib.Gallery.l2_from_host(rows) as g:
        ids, dist, dist64, _ = g.search_minkowski(q, k, "lp", 2)
        dense = g.dense64_search_l2(q, k)
        l2 = g.search_l2(q, k)
    assert np.array_equal(ids, dense[0]) and np.array_equal(_bits(dist64), _bits(dense[2])) and np.array_equal(dist, dense[1])
    assert np.array_equal(ids, l2[0]) and np.array_equal(_bits(dist64), _bits(l2[2]))


def test_query_equal_to_a_row_is_at_zero_and_first(lib):
    rows = _wide(5, 700, 131)
    q = rows[[13, 699, 0, 256]].copy()
    with lib.Gallery.from_host(rows, norm_mode=lib.NORM_NONE) as g:
        for metric, p in EXACT + (("lp", 0.5), ("lp", 3)):
            ids, dist, dist64, _ = g.search_minkowski(q, 5, metric, p)
            assert ids[:, 0].tolist() == [13, 699, 0, 256]
            assert (dist64[:, 0] == 0.0).all() and not np.signbit(dist64[:, 0]).any() and (dist64[:, 1] > 0).all()


def test_ties_go_to_the_lower_id(lib):
    """rows from {-1, 0, 1}: L1 values are small integers with huge tie classes; and a gallery of identical rows"""
    rng = np.random.default_rng(6)
    rows = rng.integers(-1, 2, (5000, 12)).astype(np.float32)
    q = rng.integers(-1, 2, (QT + 1, 12)).astype(np.float32)
    with lib.Gallery.from_host(rows, norm_mode=lib.NORM_NONE) as g:
        out = _check_exact(g, rows, q, 2048)
    ids, _, dist64, _ = out[("l1", None)]
    for i in range(q.shape[0]):
        for v in np.unique(dist64[i]):
            assert (np.diff(ids[i][dist64[i] == v]) > 0).all()
    same = np.tile(_wide(7, 1, 33), (2500, 1))
    with lib.Gallery.from_host(same, norm_mode=lib.NORM_NONE) as g:
        out = _check_exact(g, same, _wide(8, 2, 33), 2048)
    assert np.array_equal(out[("linf", None)][0], np.tile(np.arange(2048), (2, 1)))


def test_allow_bitmap_and_row_offset(lib):
    n, d, k, off = 4500, 21, 50, 1000
    rows, q = _wide(9, n, d), _wide(10, QT + 1, d)
    rng = np.random.default_rng(11)
    mask = rng.random(n) < 0.3
    few = np.zeros(n, dtype=bool)
    few[rng.choice(n, k - 1, replace=False)] = True
    with lib.Gallery.from_host(rows, norm_mode=lib.NORM_NONE, row_offset=off) as g:
        out = _check_exact(g, rows, q, k, off=off)
        assert out[("l1", None)][0].min() >= off
        _check_exact(g, rows, q, k, allow=mask, mask=mask, off=off)
        _check_exact(g, rows, q, k, allow=np.flatnonzero(mask) + off, mask=mask, off=off)          # global ids
        got = _check_exact(g, rows, q, k, allow=np.zeros(n, dtype=bool), mask=np.zeros(n, dtype=bool), off=off)
        assert (got[("l1", None)][0] == -1).all() and np.isposinf(got[("l1", None)][2]).all()
        got = _check_exact(g, rows, q, k, allow=few, mask=few, off=off)
        assert (got[("lp", 2)][0][:, :k - 1] >= off).all() and (got[("lp", 2)][0][:, k - 1] == -1).all()
        # the device entry point reads the same bitmap from device memory
        words = lib.allow_bitmap(mask, n)
        want = g.search_minkowski(q, k, "l1", allow=mask)
        dev = _device(g, q, k, "l1", None, words)
        assert np.array_equal(dev[0], want[0]) and np.array_equal(_bits(dev[2]), _bits(want[2])) and np.array_equal(dev[1], want[1])


def test_a_query_does_not_depend_on_its_batch(lib):
    n, d, k = 2600, 70, 40
    rows, q = _wide(12, n, d), _wide(13, 2 * QT + 3, d)
    with lib.Gallery.from_host(rows, norm_mode=lib.NORM_NONE) as g:
        for metric, p in EXACT + (("lp", 0.5), ("lp", 2.5)):
            whole = g.search_minkowski(q, k, metric, p)
            probe = q[5:6]
            alone = g.search_minkowski(probe, k, metric, p)
            assert np.array_equal(alone[0], whole[0][5:6]) and np.array_equal(_bits(alone[2]), _bits(whole[2][5:6]))
            for pos in range(QT + 2):                                    # every place of a tile, and the next tile
                batch = np.roll(q[:QT + 2], 1, axis=0).copy()
                batch[pos] = probe[0]
                got = g.search_minkowski(batch, k, metric, p)
                assert np.array_equal(got[0][pos], alone[0][0]) and np.array_equal(_bits(got[2][pos]), _bits(alone[2][0]))
            dev = _device(g, q, k, metric, p)
            assert np.array_equal(dev[0], whole[0]) and np.array_equal(_bits(dev[2]), _bits(whole[2])) and np.array_equal(dev[1], whole[1])


def test_gallery_kinds(lib):
    n, d, k = 2100, 45, 30
    rows, q = _wide(14, n, d), _wide(15, QT + 1, d)
    with lib.Gallery.from_host(rows, norm_mode=lib.NORM_NONE) as g, lib.Gallery.l2_from_host(rows) as gl:
        a, b = _check_exact(g, rows, q, k), _check_exact(gl, rows, q, k)     # (on L2 only the caller's d columns count)
        for key in a:
            assert np.array_equal(a[key][0], b[key][0]) and np.array_equal(_bits(a[key][2]), _bits(b[key][2]))
    unit, qu = _gauss(16, n, d), _gauss(17, 3, d)
    with lib.Gallery.from_host(unit, norm_mode=lib.NORM_L2) as g:
        stored = g.get_rows(0, n)
        assert not np.array_equal(stored, unit)
        _check_exact(g, stored, qu, k)


def test_after_remove_and_append(lib):
    n, d, k = 2300, 18, 25
    rows, more, q = _wide(18, n, d), _wide(19, 300, d), _wide(20, 3, d)
    g = lib.Gallery.l2_from_host(rows, capacity=n + 300)
    try:
        _check_exact(g, rows, q, k)
        gone = np.random.default_rng(21).choice(n, 700, replace=False)
        kept = g.remove(gone)
        _check_exact(g, rows[kept], q, k)
        g.append(more)
        _check_exact(g, np.concatenate([rows[kept], more]), q, k)
    finally:
        g.close()


def test_argument_checks_of_the_library(lib):
    import ctypes as C
    L = lib.load()
    rows = _gauss(22, 10, 4)
    q = _gauss(23, 2, 4)
    idx = np.zeros((2, 3), np.int64)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    with lib.Gallery.from_host(rows, norm_mode=lib.NORM_NONE) as g:
        call = lambda metric, p, k, nq=2: L.mi_knn_search_minkowski(g._h, P(q), nq, 0, 4, 1, metric, p, k, None, 0, P(idx), None, None, None)
        for metric, p, k in ((0, 1.0, 3), (4, 1.0, 3), (3, 0.0, 3), (3, -2.0, 3), (3, float("nan"), 3), (3, float("inf"), 3),
                             (1, 1.0, 0), (1, 1.0, 2049)):
            assert call(metric, p, k) == lib.MI_ERR_INVALID
        idx[:] = -5
        assert call(1, 0.0, 3, nq=0) == 0 and (idx == -5).all()                 # nq == 0: MI_OK, nothing written
        assert call(2, float("nan"), 3) == 0                                      # p is ignored unless the metric is MI_MINK_LP
        assert L.mi_knn_search_minkowski_device(g._h, None, 0, 1, 0.0, 3, None, None, None, None, None) == 0
        ids, dist, dist64, _ = g.search_minkowski(q, 3, "linf")
        assert np.array_equal(ids, idx)
        only = g.search_minkowski(q.astype(np.float64), 3, "linf")                           # float64 queries round to f32
        assert np.array_equal(only[0], ids) and np.array_equal(_bits(only[2]), _bits(dist64))


def test_query_layouts_give_the_contiguous_answer(lib):
    """every layout and element type of tests/_layouts.py (transposed, padded, column-strided, offset, broadcast; float32 and
    float64) gives the bits of the contiguous float32 queries; float64 queries beyond float32 are rounded to it"""
    n, k = 700, 20
    for nq, d in ((7, 5), (QT + 1, 37), (1, 37), (3, 130)):
        rows, q = _wide(26, n, d), _wide(27, nq, d)
        with lib.Gallery.from_host(rows, norm_mode=lib.NORM_NONE) as g:
            for metric, p in (("l1", None), ("lp", 0.5)):
                call = lambda x: g.search_minkowski(x, k, metric, p)[:3]
                want = call(q)
                for lay in L.layouts(q, np.nan, bcast=True):
                    ref = want if lay.name != "bcast32" else call(L.expected(lay, q))
                    L.same(call(lay.view), ref, "%s p=%s, %d x %d, %s" % (metric, p, nq, d, lay.name))
                q64 = L.beyond_float32(q, [0, nq - 1], [0, d - 1])
                L.same(call(q64), want, "%s p=%s, %d x %d, float64 beyond float32" % (metric, p, nq, d))


# ---------------------------------------------------------------------------------------------- Lp against the reference
LP_INPUTS = [(n, d, seed) for (n, d) in ((3000, 100), (2500, 259)) for seed in (0, 1, 2)]
_lp_cache = {}


def _lp_case(n, d, seed, p, k=128):
    key = (n, d, seed, p)
    if key not in _lp_cache:
        rows, q = _gauss(100 + seed, n, d), _gauss(200 + seed, 8, d)
        _lp_cache[key] = (rows, q) + T.lp_reference_topk(rows, q, p, k)
    return _lp_cache[key]


@pytest.mark.parametrize("p", [0.5, 1.5, 3])
def test_lp_against_reference(lib, p):
    k, worst = 128, 0.0
    tol = 8 * LP_MEASURED[p]
    assert tol <= LP_CAP
    for n, d, seed in LP_INPUTS:
        rows, q, rid, rval = _lp_case(n, d, seed, p)
        gap = T.min_relative_gap(rval)
        assert gap >= 1e-9, "the reference's own values lie %.3g apart at n=%d d=%d seed=%d: pick another seed" % (gap, n, d, seed)
        with lib.Gallery.from_host(rows, norm_mode=lib.NORM_NONE) as g:
            ids, dist, dist64, _ = g.search_minkowski(q, k, "lp", p)
        dev = float((np.abs(dist64 - rval[:, :k]) / rval[:, :k]).max())
        worst = max(worst, dev)
        if p == 0.5:                                                    # (a figure for DESIGN.md, no condition)
            lane = T.topk(T.values(rows, q, "lp", p), k)[1]
            print("lp p=0.5: bits equal to the lane-order sum of numpy's correctly rounded sqrt: %s"
                  % np.array_equal(_bits(dist64), _bits(lane)))
        print("lp p=%s n=%d d=%d seed=%d: min gap %.3g, max relative deviation %.3g, bit-equal %s"
              % (p, n, d, seed, gap, dev, np.array_equal(_bits(dist64), _bits(rval[:, :k]))))
        assert np.array_equal(ids, rid[:, :k])
        assert dev <= tol
        assert np.array_equal(dist, dist64.astype(np.float32))
    print("lp p=%s: largest relative deviation %.3g (tolerance %.3g)" % (p, worst, tol))


def test_fractional_matchers(lib):
    from isehr_amd import nnsearch
    n, d, nq, K = 2500, 64, 20, 12
    train, test = _gauss(300, n, d) + 0.25, _gauss(301, nq, d) + 0.25
    tu, qu = T.unit_rows(train), T.unit_rows(test)
    _, rval = T.lp_reference_topk(tu, qu, 0.5, K)
    assert T.min_relative_gap(rval) >= 1e-9
    want = np.argsort(T.fractional_distance(qu, tu, 0.5), axis=1, kind="stable")[:, :K]
    idx, per_query = nnsearch.matching_fractional_dis_hip(K, train, test, p=0.5)
    assert idx.dtype == np.int64 and idx.shape == (min(nq, K), K) and per_query > 0        # the reference's slice of the QUERY axis
    assert np.array_equal(idx, want[:K])
    idx, per_query = nnsearch.MATCHING_METHODS["Lp"](K, train, test)
    assert idx.dtype == np.int64 and idx.shape == (nq, K) and per_query > 0
    assert np.array_equal(idx, want)
    with pytest.raises(RuntimeError):
        nnsearch.MATCHING_METHODS["Lp"](n + 1, train, test[:2])


def test_knn_wrapper(lib):
    from isehr_amd.knn import KNN
    n, d, k = 1200, 30, 20
    for method, p in (("l1", None), ("linf", None), ("lp", 0.5)):
        x, q = (_gauss(24, n, d), _gauss(25, 5, d)) if method == "lp" else (_wide(24, n, d), _wide(25, 5, d))
        knn = KNN(x, method, p=p)
        try:
            dist, ids = knn.search(q, k)
            if method == "lp":
                rid, rval = T.lp_reference_topk(x, q, p, k)
                assert T.min_relative_gap(rval) >= 1e-9
                assert np.array_equal(ids, rid[:, :k]) and (np.abs(dist - rval[:, :k]) <= 2.0 ** -23 * rval[:, :k]).all()
            else:
                tid, tval = T.topk(T.values(x, q, method), k)
                assert np.array_equal(ids, tid) and np.array_equal(dist, tval.astype(np.float32))
            assert dist.dtype == np.float32 and (np.diff(dist.astype(np.float64), axis=1) >= 0).all()
            gone = ids[:, 0]
            assert knn.remove_ids(gone) == np.unique(gone).size and knn.N == n - np.unique(gone).size
            left = np.delete(x, np.unique(gone), axis=0)
            dist, ids = knn.search(q, k)
            if method == "lp":
                rid, rval = T.lp_reference_topk(left, q, p, k)
                assert T.min_relative_gap(rval) >= 1e-9
                assert np.array_equal(ids, rid[:, :k])
            else:
                tid, tval = T.topk(T.values(left, q, method), k)
                assert np.array_equal(ids, tid) and np.array_equal(dist, tval.astype(np.float32))
            with pytest.raises(NotImplementedError):
                knn.range_search(q, 1.0)
        finally:
            knn.close()
