"""GPU: range search (mi_range_search, csrc/api_range.hip, csrc/range_select.hip, csrc/csr_order.hip) pinned to the exact answer
on lattice data.

The data of tests/_lattice_truth.py scores exactly in every number format and summation order (test_lattice_truth_cpu.py), so
the host truth is the device's answer to the bit and the contract at the top of api_range.hip is asserted with ==: every row
whose exact score is >= min_score, ordered by (score desc, row asc), scores as f32 bits.  No band, no excluded row.  Before any
answer is judged the gallery must hold the rows it was given bit for bit (Gallery.get_rows)."""
import ctypes as C

import numpy as np
import pytest

import _lattice_truth as lt

pytestmark = pytest.mark.gpu

INF = float("inf")


def _same(got, want, what=""):
    """lims, idx and the score bits of two answers are equal"""
    lg, ig, sg = got[:3]
    lw, iw, sw = want[:3]
    assert lg.dtype == np.int64 and ig.dtype == np.int64 and sg.dtype == np.float32
    if not np.array_equal(lg, lw):
        q = int(np.flatnonzero(np.diff(lg) != np.diff(lw))[0])
        raise AssertionError("%s: query %d has %d hits, the truth has %d" % (what, q, np.diff(lg)[q], np.diff(lw)[q]))
    if not np.array_equal(ig, iw):
        p = int(np.flatnonzero(ig != iw)[0])
        q = int(np.searchsorted(lw, p, side="right") - 1)
        raise AssertionError("%s: query %d, position %d: row %d (score %r), the truth has row %d (score %r)"
                             % (what, q, p - lw[q], ig[p], sg[p], iw[p], sw[p]))
    assert np.array_equal(sg.view(np.uint32), sw.view(np.uint32)), "%s: score bits differ" % what


def _ask(g, Q, tau, **kw):
    return g.range_search(Q, tau, **kw)[:3]


def _truth(S, tau, row_offset=0):
    lims, ids, sc = lt.range_truth(S, tau)
    return lims, ids + row_offset, sc


def _stored_bit_for_bit(g, X):
    R = g.get_rows(0, g.n)
    assert g.n == len(X) and R.dtype == np.float32
    assert np.array_equal(R.view(np.uint32), np.ascontiguousarray(X).view(np.uint32)), "the gallery does not hold the rows it was given"


def _gallery(X, norm=None, **kw):
    from isehr_amd import _lib
    g = _lib.Gallery.from_host(X, norm_mode=_lib.NORM_NONE if norm is None else norm, **kw)
    try:
        _stored_bit_for_bit(g, X)
    except BaseException:
        g.close()
        raise
    return g


def _queries(rng, planted, nq, d):
    """the planted one-hot queries, then dense ones (every coordinate non-zero) up to nq; at least one of each when nq >= 2"""
    keep = planted[:max(1, nq - max(1, nq // 4))] if nq >= 2 else planted[:1]
    return np.concatenate([keep, lt.dense_queries(rng, nq - len(keep), d)]) if nq > len(keep) else keep


def _taus(S, L):
    """the thresholds of the issue around the integer level L (which has rows exactly at it) and at the ends"""
    return [float(L), float(np.nextafter(float(L), INF)), float(np.nextafter(float(L), -INF)), 0.0, -0.0,
            float(S.max()) + 1.0, -INF, INF]


# one d per n, every nq of the list; d = 1 is accepted by the gallery
SHAPES = [(1, 1, 1), (1, 32, 256), (255, 32, 257), (256, 100, 2), (257, 1, 255), (513, 32, 256), (600, 100, 257)]


@pytest.mark.parametrize("n, d, nq", SHAPES)
def test_shapes_and_thresholds(n, d, nq):
    rng = np.random.default_rng(1000 * n + d)
    L = 1
    counts = [(n, n)] if n == 1 else [(n // 3, n // 7), (n, n // 2), (0, 0), (1, 1), (n - 1, n - 1)][:d]
    X, P = lt.planted_gallery(rng, n, d, L, counts)
    Q = _queries(rng, P, nq, d)
    S = lt.int_scores(X, Q)
    assert Q.shape == (nq, d) and (S[0] == L).sum() == counts[0][1] > 0          # rows exactly at the level
    assert (S == 0).any() or n == 1
    g = _gallery(X)
    try:
        answers = {}
        for tau in _taus(S, L):
            got = _ask(g, Q, tau)
            _same(got, _truth(S, tau), "n %d d %d nq %d tau %r" % (n, d, nq, tau))
            answers[repr(tau)] = got
        # rows at L are in at L and just below it, out just above it
        at, above, below = (np.diff(answers[repr(t)][0]) for t in _taus(S, L)[:3])
        assert np.array_equal(at, (S >= L).sum(1)) and np.array_equal(below, at) and np.array_equal(above, (S > L).sum(1))
        assert above[0] == at[0] - counts[0][1]
        _same(answers["0.0"], answers["-0.0"], "tau 0.0 against -0.0")
        assert np.array_equal(np.diff(answers["0.0"][0]), (S >= 0).sum(1))
        for empty in (repr(float(S.max()) + 1.0), repr(INF)):
            assert not answers[empty][0].any() and len(answers[empty][1]) == 0 and len(answers[empty][2]) == 0
        assert (np.diff(answers[repr(-INF)][0]) == n).all()
    finally:
        g.close()


def test_unit_lattice_norm_l2():
    """NORM_L2: rows and queries of norm exactly 1, scores multiples of 1/32.  The ingest must keep the bits (asserted)."""
    from isehr_amd import _lib
    rng = np.random.default_rng(64)
    n, nq = 600, 40
    X = lt.unit_rows(rng, n)
    Q = lt.unit_rows(rng, nq)
    copies = {0: [3, 255, 256, 599], 7: [100], 39: [5, 6, 7]}
    for q, rows in copies.items():
        X[rows] = Q[q]
    X[300] = -Q[0]
    S = lt.unit_scores(X, Q)
    g = _gallery(X, norm=_lib.NORM_L2)
    try:
        levels = np.unique(S)
        mid = float(levels[levels > 0][1])                   # a level with rows exactly at it, a small multiple of 1/32
        assert (S == mid).any() and 0 < mid < 1 and mid * 32 == round(mid * 32)
        for tau in (-1.0, 1.0, mid, float(np.nextafter(mid, INF)), float(np.nextafter(mid, -INF)), 0.0, -0.0,
                    float(np.nextafter(1.0, INF)), -INF, INF):
            got = _ask(g, Q, tau)
            _same(got, _truth(S, tau), "unit lattice, tau %r" % tau)
            if tau == -1.0:
                assert (np.diff(got[0]) == n).all()
            if tau == 1.0:                                    # exactly the copies of the query
                for q in range(nq):
                    assert got[1][got[0][q]:got[0][q + 1]].tolist() == sorted(copies.get(q, []))
    finally:
        g.close()


@pytest.fixture(scope="module")
def runs():
    """BOUNDARY_N x 32 rows; queries with exactly 0, 1, 2047, 2048, 2049, 4096, 4097 and n hits at tau = 1, then dense ones"""
    rng = np.random.default_rng(4200)
    n, d, tau = lt.BOUNDARY_N, 32, 1
    X, P = lt.planted_gallery(rng, n, d, tau, lt.BOUNDARY_COUNTS)
    Q = np.concatenate([P, lt.dense_queries(rng, 4, d)])
    S = lt.int_scores(X, Q)
    g = _gallery(X)
    yield g, X, Q, S, tau
    g.close()


def test_run_boundaries(runs):
    g, X, Q, S, tau = runs
    n = len(X)
    want = _truth(S, tau)
    hits = np.diff(want[0])
    # the hit counts and the tie classes across the run boundaries come from the truth, before the device is asked
    assert hits[:8].tolist() == [0, 1, 2047, 2048, 2049, 4096, 4097, n] and n >= 4200
    for q in range(8):
        sc = want[2][want[0][q]:want[0][q + 1]]
        ids = want[1][want[0][q]:want[0][q + 1]]
        for edge in (lt.RANGE_RUN, 2 * lt.RANGE_RUN):
            if hits[q] > edge:                               # equal scores on both sides of the edge, ids ascending across it
                assert sc[edge - 2] == sc[edge - 1] == sc[edge] and ids[edge - 2] < ids[edge - 1] < ids[edge]
    _same(_ask(g, Q, tau), want, "run boundaries")
    for q in range(len(Q)):                                  # single queries: max_cnt is that query's own count
        _same(_ask(g, Q[q:q + 1], tau), _truth(S[q:q + 1], tau), "run boundaries, query %d alone" % q)
    _same(_ask(g, Q, -INF), _truth(S, -INF), "every row of every query")


def test_signed_scores_through_two_merge_passes():
    """The hits are keyed by the complement of the score's key and ordered ascending (csrc/csr_order.hip): one query whose hits
    span negative, zero and positive scores in five tie classes of hundreds of rows each, more than three runs of them (four
    sorted runs, two merge passes), beside a query with no hit and one with exactly one."""
    run = lt.RANGE_RUN
    rng = np.random.default_rng(8229)
    n, d, tau = 4 * run + 37, 32, -1
    X, Q = lt.planted_gallery(rng, n, d, tau, [(3 * run + 356, 900), (0, 0), (1, 1)])
    S = lt.int_scores(X, Q)
    want = _truth(S, tau)
    hits = np.diff(want[0])
    sc0 = want[2][:hits[0]]
    classes, sizes = np.unique(sc0, return_counts=True)
    # the truth first: more than three runs of hits, classes below, at and above zero, each of hundreds of rows
    assert hits.tolist() == [3 * run + 356, 0, 1] and hits[0] > 3 * run
    assert classes.tolist() == [-1.0, 0.0, 1.0, 2.0, 3.0] and (sizes >= 900).all()
    g = _gallery(X)
    try:
        got = _ask(g, Q, float(tau))
        _same(got, want, "signed scores, two merge passes")
        ids0, got0 = got[1][:hits[0]], got[2][:hits[0]]
        assert (np.diff(got0) <= 0).all()                    # descending across zero
        for v in classes:
            assert (np.diff(ids0[got0 == v]) > 0).all()      # ids ascend inside every tie class
        for q in range(3):
            _same(_ask(g, Q[q:q + 1], float(tau)), _truth(S[q:q + 1], tau), "signed scores, query %d alone" % q)
    finally:
        g.close()


def test_chunk_ladder(runs):
    """survivor_cap 1024: a query with more than 1024 survivors in a chunk makes the chunk overflow and be done again in halves"""
    g, X, Q, S, tau = runs
    ref = {t: _ask(g, Q, t) for t in (tau, -INF)}
    cap0 = g.get_option("survivor_cap")
    assert cap0 >= len(X)                                    # the default cap holds every row: no overflow above
    try:
        g.set_option("survivor_cap", 1024)
        for t in (tau, -INF):
            before = g.status()["overflow_batches"]
            got = _ask(g, Q, t)
            assert g.status()["overflow_batches"] > before
            _same(got, _truth(S, t), "survivor_cap 1024, tau %r" % t)
            _same(got, ref[t], "survivor_cap 1024 against the default, tau %r" % t)
        # 300 queries (the tile kernel), every row a hit
        Q300 = np.concatenate([Q, lt.dense_queries(np.random.default_rng(1), 300 - len(Q), Q.shape[1])])
        S300 = lt.int_scores(X, Q300)
        before = g.status()["overflow_batches"]
        got = _ask(g, Q300, -INF)
        assert g.status()["overflow_batches"] > before
        _same(got, _truth(S300, -INF), "survivor_cap 1024, 300 queries, every row")
    finally:
        g.set_option("survivor_cap", cap0)
    _same(_ask(g, Q300, -INF), got, "300 queries at the default cap")


def test_paths(runs):
    g, X, Q, S, tau = runs
    want = _truth(S, tau)
    ref = _ask(g, Q, tau)
    _same(ref, want, "default path")
    img0 = int(g.get_option("image_dtype"))
    try:
        for img in (0, 1):                                   # bf16 image, fp16 image
            g.set_image_dtype(img)
            _same(_ask(g, Q, tau), want, "image_dtype %d" % img)
            for sbk in (0, 1):                               # <= 128 queries: tile kernel / streaming kernel
                g.set_option("small_batch_kernel", sbk)
                _same(_ask(g, Q, tau), want, "image_dtype %d, small_batch_kernel %d" % (img, sbk))
            g.set_option("force_exact", 1)                   # f32 scorer
            _same(_ask(g, Q, tau), want, "image_dtype %d, force_exact" % img)
            g.set_option("force_exact", 0)
    finally:
        g.set_image_dtype(img0)
        g.set_option("force_exact", 0)
        g.set_option("small_batch_kernel", 1)
    _same(_ask(g, Q, tau), ref, "options restored")


def test_query_dtypes_and_strides(runs):
    g, X, Q, S, tau = runs
    want = _truth(S, tau)
    Q64 = Q.astype(np.float64)
    wide = np.zeros((len(Q), 2 * Q.shape[1]), np.float32)
    wide[:, ::2] = Q
    wide[:, 1::2] = 7.0                                      # what a wrong stride would read
    view = wide[:, ::2]
    assert view.strides[1] == 8 and np.array_equal(view, Q)
    _same(_ask(g, Q64, tau), want, "float64 queries")
    _same(_ask(g, view, tau), want, "column-strided queries")
    wide64 = wide.astype(np.float64)
    _same(_ask(g, wide64[:, ::2], tau), want, "column-strided float64 queries")


@pytest.fixture(scope="module")
def small():
    """300 rows and 1025 queries: two batches, the second of one query"""
    rng = np.random.default_rng(300)
    n, d, tau = 300, 32, 1
    X, P = lt.planted_gallery(rng, n, d, tau, [(0, 0), (n, 100), (1, 1), (256, 90), (257, 90)])
    Q = np.concatenate([P, lt.dense_queries(rng, 1025 - len(P), d)])
    Q[1024] = P[1]                                           # the lone query of the second batch: every row is a hit
    S = lt.int_scores(X, Q)
    g = _gallery(X)
    yield g, X, Q, S, tau
    g.close()


@pytest.mark.parametrize("nq", [1024, 1025])
def test_batches_and_capacity(small, nq):
    from isehr_amd import _lib
    g, X, Q, S, tau = small
    q = np.ascontiguousarray(Q[:nq])
    want = _truth(S[:nq], tau)
    total = int(want[0][-1])
    assert total > nq and (nq < 1025 or want[0][-1] - want[0][-2] == len(X))
    _same(_ask(g, q, tau), want, "%d queries" % nq)
    _same(_ask(g, q, tau, max_results=5), want, "%d queries through the binding's second call" % nq)
    P = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    lib = _lib.load()
    lims = np.full(nq + 1, -7, np.int64)
    idx = np.full(total, -3, np.int64)
    sc = np.full(total, 5.0, np.float32)
    rc = lib.mi_range_search(g._h, P(q), nq, _lib.MI_F32, q.shape[1], 1, float(tau), total - 1, P(lims), P(idx), P(sc), None)
    assert rc == _lib.MI_ERR_CAPACITY
    assert np.array_equal(lims, want[0])                     # lims complete
    assert (idx == -3).all() and (sc == 5.0).all()           # the output arrays untouched
    rc = lib.mi_range_search(g._h, P(q), nq, _lib.MI_F32, q.shape[1], 1, float(tau), total, P(lims), P(idx), P(sc), None)
    assert rc == 0
    _same((lims, idx, sc), want, "%d queries at max_results = total" % nq)


def test_ids_offset_append_remove():
    from isehr_amd import _lib
    rng = np.random.default_rng(600)
    n, d, tau, off = 600, 32, 1, 2 ** 33
    X, P = lt.planted_gallery(rng, n, d, tau, [(n // 2, 100), (n, 200), (1, 1), (0, 0)])
    Q = np.concatenate([P, lt.dense_queries(rng, 6, d)])
    S = lt.int_scores(X, Q)
    g = _gallery(X)
    go = _gallery(X, row_offset=off)
    ga = _lib.Gallery.empty(n, d, norm_mode=_lib.NORM_NONE, row_offset=off)
    fresh = None
    try:
        want = _truth(S, tau)
        _same(_ask(g, Q, tau), want, "one-shot gallery")
        assert go.row_offset == off
        _same(_ask(go, Q, tau), _truth(S, tau, off), "row_offset 2**33")
        ga.append(X[:300])                                   # 300 and 600 rows: both appends end inside a tile
        _stored_bit_for_bit(ga, X[:300])
        _same(_ask(ga, Q, tau), _truth(S[:, :300], tau, off), "after the first append")
        ga.append(X[300:])
        _stored_bit_for_bit(ga, X)
        _same(_ask(ga, Q, tau), _truth(S, tau, off), "after the second append")
        # remove rows that were hits (every other hit of query 0, the one hit of query 2, the first and the last row)
        hits0 = want[1][want[0][0]:want[0][1]]
        gone = np.unique(np.concatenate([hits0[::2], want[1][want[0][2]:want[0][3]], [0, n - 1]]))
        kept = g.remove(gone)
        assert np.array_equal(kept, np.setdiff1d(np.arange(n), gone))
        _stored_bit_for_bit(g, X[kept])
        fresh = _gallery(np.ascontiguousarray(X[kept]))
        for t in (tau, -INF):
            got = _ask(g, Q, t)
            _same(got, _truth(S[:, kept], t), "after remove, tau %r" % t)
            _same(got, _ask(fresh, Q, t), "after remove against a fresh gallery of the survivors, tau %r" % t)
    finally:
        for h in (g, go, ga, fresh):
            if h is not None:
                h.close()


def test_two_batch_capacity_protocol(small):
    """nq = QB + 1 (QB = 1024 queries a batch, api_internal.h): the ordering stage's device-side guard is given the batch's room;
    one entry short, whichever batch runs out, the call returns MI_ERR_CAPACITY with out_lims complete and out_idx untouched,
    and at max_results = total it succeeds"""
    from isehr_amd import _lib
    g, X, Q, S, tau = small
    nq = 1025
    q = np.ascontiguousarray(Q[:nq])
    want = _truth(S[:nq], tau)
    total, first = int(want[0][-1]), int(want[0][1024])
    assert 0 < first < total                                 # both batches have hits
    P = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    lib = _lib.load()
    for cap in (total - 1, first, first - 1, 1, 0):          # the second batch does not fit; the first does not fit
        lims = np.full(nq + 1, -7, np.int64)
        idx = np.full(total, -3, np.int64)
        sc = np.full(total, 5.0, np.float32)
        rc = lib.mi_range_search(g._h, P(q), nq, _lib.MI_F32, q.shape[1], 1, float(tau), cap, P(lims), P(idx), P(sc), None)
        assert rc == _lib.MI_ERR_CAPACITY, cap
        assert np.array_equal(lims, want[0])                 # lims complete
        assert (idx == -3).all() and (sc == 5.0).all()       # the output arrays untouched
    rc = lib.mi_range_search(g._h, P(q), nq, _lib.MI_F32, q.shape[1], 1, float(tau), total, P(lims), P(idx), P(sc), None)
    assert rc == 0
    _same((lims, idx, sc), want, "two batches at max_results = total")
