"""GPU: filtered top-K (mi_knn_search_filtered, csrc/api_filter.hip, csrc/filter_select.hip) pinned to the exact answer on the
integer lattice of tests/_lattice_truth.py.

Every score is exact in every number format and order, the tie classes hold a seventh of the gallery, so the K boundary always
falls inside a tie and the contract at the top of api_filter.hip is asserted with ==: the first k allowed rows in the order
(score desc, row asc), ids and score bits, padded with -1 / -inf.  filter_path 0, 1 and 2 must agree bit for bit, and so must a
second call with the sub-gallery cached.  The gallery must hold the rows it was given bit for bit before anything is judged."""
import math

import numpy as np
import pytest

import _lattice_truth as lt

pytestmark = pytest.mark.gpu


def _same(got, want, what=""):
    ig, sg = got[:2]
    iw, sw = want[:2]
    assert ig.dtype == np.int64 and sg.dtype == np.float32 and ig.shape == iw.shape and sg.shape == sw.shape
    if not np.array_equal(ig, iw):
        q, j = (int(v[0]) for v in np.nonzero(ig != iw))
        raise AssertionError("%s: query %d, position %d: row %d (score %r), the truth has row %d (score %r)"
                             % (what, q, j, ig[q, j], sg[q, j], iw[q, j], sw[q, j]))
    assert np.array_equal(sg.view(np.uint32), sw.view(np.uint32)), "%s: score bits differ" % what


def _gallery(X, **kw):
    from isehr_amd import _lib
    g = _lib.Gallery.from_host(X, norm_mode=_lib.NORM_NONE, **kw)
    try:
        R = g.get_rows(0, g.n)
        assert np.array_equal(R.view(np.uint32), np.ascontiguousarray(X).view(np.uint32)), "the gallery does not hold the rows it was given"
    except BaseException:
        g.close()
        raise
    return g


def _run(g, Q, k, allow=None, path=0, allow_ptr=None):
    g.set_option("filter_path", path)
    try:
        idx, sc, _, info = g.search_filtered(Q, k, allow, allow_ptr=allow_ptr)
    finally:
        g.set_option("filter_path", 0)
    return idx, sc, info


def _kprime(g, k, allowed):
    """the over-fetch depth as api_filter.hip states it"""
    want = math.ceil(1.25 * k / (allowed / g.n)) + 32
    return min(want, 2048, int(g.get_option("rescore_cap")), int(g.get_option("survivor_cap")) // 4, g.n)


def _every_path(g, Q, S, k, mask, what, row_offset=0):
    """paths 0, 1 and 2, each twice (the second call may reuse the cached sub-gallery), against the truth -> the three infos"""
    want = lt.filtered_truth(S, mask, k, row_offset)
    allowed = int(mask.sum())
    infos = []
    for path in (0, 1, 2):
        for again in (0, 1):
            idx, sc, info = _run(g, Q, k, mask, path)
            _same((idx, sc), want, "%s, k %d, path %d, call %d" % (what, k, path, again))
            assert info["allowed"] == allowed
            if allowed == 0 or path:
                assert info["path"] == (path if allowed else 0)
            if path == 1 and again and allowed:
                assert info["cache_hit"] == 1
        infos.append(info)
    if allowed == 0:
        assert (want[0] == -1).all() and np.isneginf(want[1]).all()
    return infos


def _masks(n, k):
    """name -> bool mask [n]: the masks of the issue that exist at this n"""
    out = {"none": np.zeros(n, bool), "all": np.ones(n, bool), "every other": np.arange(n) % 2 == 0}
    for name, row in (("first", 0), ("last", n - 1), ("in the last partial tile", n - 1 - (n - 1) % 256 + ((n - 1) % 256) // 2)):
        out["only the " + name + " row"] = np.arange(n) == row
    rng = np.random.default_rng(n)
    for m in (k - 1, k, k + 1):
        if 0 < m <= n:
            mk = np.zeros(n, bool)
            mk[rng.choice(n, m, replace=False)] = True
            out["%d rows" % m] = mk
    edges = [r for r in (31, 32, 63, 64) if r < n]
    if edges:
        mk = np.zeros(n, bool)
        mk[edges] = True
        out["word edges"] = mk
    return out


@pytest.mark.parametrize("n, d, nq, k", [(1, 1, 3, 1), (257, 32, 9, 5), (600, 100, 130, 5)])
def test_masks(n, d, nq, k):
    rng = np.random.default_rng(7 * n)
    X, P = lt.planted_gallery(rng, n, d, 1, [(n, (n + 1) // 2)] if n < 3 else [(n // 2, n // 4), (n, n // 2), (k, k)][:d])
    Q = np.concatenate([P, lt.dense_queries(rng, nq - len(P), d)])
    S = lt.int_scores(X, Q)
    g = _gallery(X)
    try:
        for name, mask in _masks(n, k).items():
            infos = _every_path(g, Q, S, k, mask, "n %d, %s" % (n, name))
            if name == "none":
                assert all(i["allowed"] == 0 and i["path"] == 0 for i in infos)
            if name == "all":                                # must equal the unfiltered search bit for bit
                ref = g.search(Q, k)[:2]
                for path in (0, 1, 2):
                    _same(_run(g, Q, k, mask, path), ref, "n %d, all rows against search, path %d" % (n, path))
                assert infos[2]["rerun_queries"] == 0
    finally:
        g.close()


def test_k_values():
    """k in {1, 2, allowed, allowed + 1, 2048} on a gallery of fewer than 2048 rows"""
    rng = np.random.default_rng(77)
    n, d, nq = 600, 32, 12
    X, P = lt.planted_gallery(rng, n, d, 1, [(n // 2, n // 4), (n, n // 2)])
    Q = np.concatenate([P, lt.dense_queries(rng, nq - len(P), d)])
    S = lt.int_scores(X, Q)
    mask = np.zeros(n, bool)
    mask[rng.choice(n, 150, replace=False)] = True
    allowed = int(mask.sum())
    g = _gallery(X)
    try:
        for k in (1, 2, allowed, allowed + 1, 2048):
            _every_path(g, Q, S, k, mask, "%d allowed of %d" % (allowed, n))
        idx, sc, _ = _run(g, Q, 2048, mask, 2)
        assert (idx[:, allowed:] == -1).all() and (idx[:, :allowed] >= 0).all()
    finally:
        g.close()


@pytest.fixture(scope="module")
def ties():
    """2600 x 32 rows, rows [0, 1500) disallowed, k = 10.  One-hot queries on planted columns:
      0 blocked    every disallowed row outscores every allowed row: the over-fetch finds no allowed row at depth K' < n
      1 tie        5 allowed rows at 3; at 2 a class of 40 disallowed rows (the lower ids) and 40 allowed rows: the answer takes
                   the 5 lowest allowed ids of the class; certified by the over-fetch
      2 one short  k - 1 allowed rows at 3, then 100 disallowed rows at 2, every other row <= 0: the top K' holds k - 1 allowed
                   rows, the k-th comes from below and only the compact path finds it
    and random columns / dense queries, which the over-fetch certifies."""
    rng = np.random.default_rng(2600)
    n, d, k, cut = 2600, 32, 10, 1500
    X = lt.int_rows(rng, n, d)
    mask = np.arange(n) >= cut
    low = lambda m: rng.integers(lt.LO, 1, size=m).astype(np.float32)   # noqa: E731  levels -3 .. 0
    X[:cut, 0] = rng.integers(1, lt.HI + 1, size=cut)
    X[cut:, 0] = low(n - cut)
    X[:, 1] = low(n)
    X[rng.choice(np.arange(cut, n), 45, replace=False), 1] = 2
    X[rng.choice(np.flatnonzero(mask & (X[:, 1] == 2)), 5, replace=False), 1] = 3
    X[rng.choice(cut, 40, replace=False), 1] = 2
    X[:, 2] = low(n)
    X[rng.choice(np.arange(cut, n), k - 1, replace=False), 2] = 3
    X[rng.choice(cut, 100, replace=False), 2] = 2
    Q = np.zeros((8, d), np.float32)
    Q[np.arange(8), np.arange(8)] = [1, 1, 1, 1, 2, 3, 1, 2]
    Q = np.concatenate([Q, lt.dense_queries(rng, 4, d)])
    S = lt.int_scores(X, Q)
    g = _gallery(X)
    yield g, X, Q, S, mask, k
    g.set_option("filter_path", 0)
    g.close()


def _uncertified(S, mask, k, kp):
    """queries whose first kp rows in (score desc, row asc) order hold fewer than k allowed rows"""
    n = S.shape[1]
    if kp >= n:
        return np.zeros(len(S), bool)
    return np.array([mask[np.lexsort((np.arange(n), -row))[:kp]].sum() < k for row in S])


def test_ties_at_k_and_certification(ties):
    g, X, Q, S, mask, k = ties
    n = len(X)
    want = lt.filtered_truth(S, mask, k)
    # the construction, from the truth
    assert S[0][~mask].min() > S[0][mask].max()
    cls = np.flatnonzero(S[1] == 2)
    assert (~mask[cls]).sum() == 40 and mask[cls].sum() == 40 and cls[~mask[cls]].max() < cls[mask[cls]].min()
    assert (want[1][1] == [3] * 5 + [2] * 5).all() and want[0][1][5:].tolist() == cls[mask[cls]][:5].tolist()
    assert (S[2][mask] == 3).sum() == k - 1 and want[1][2][k - 1] <= 0
    kp = _kprime(g, k, int(mask.sum()))
    assert kp < n
    expect = _uncertified(S, mask, k, kp)
    assert expect[0] and not expect[1] and expect[2] and 0 < expect.sum() < len(Q)     # both kinds in one call
    infos = _every_path(g, Q, S, k, mask, "ties")
    assert infos[1]["path"] == 1 and infos[2]["path"] == 2
    assert infos[2]["kprime"] == kp and infos[2]["rerun_queries"] == expect.sum()
    # single queries on path 2: who answered is reported
    for q in (0, 1, 2):
        idx, sc, info = _run(g, Q[q:q + 1], k, mask, 2)
        _same((idx, sc), (want[0][q:q + 1], want[1][q:q + 1]), "ties, query %d alone, path 2" % q)
        assert info["path"] == 2 and info["rerun_queries"] == int(expect[q])


def test_ids_and_bitmaps():
    import torch
    from isehr_amd import _lib
    rng = np.random.default_rng(88)
    n, d, k, off = 600, 32, 7, 2 ** 33
    X = lt.int_rows(rng, n, d)
    Q = np.concatenate([np.eye(d, dtype=np.float32)[:4] * 2, lt.dense_queries(rng, 5, d)])
    S = lt.int_scores(X, Q)
    mask = rng.random(n) < 0.4
    g = _gallery(X, row_offset=off)
    try:
        assert g.row_offset == off
        want = lt.filtered_truth(S, mask, k, off)
        _every_path(g, Q, S, k, mask, "row_offset 2**33", row_offset=off)
        words = _lib.allow_bitmap(mask, n)
        assert np.array_equal(np.asarray(_lib.allow_bitmap(off + np.flatnonzero(mask), n, off)), np.asarray(words))
        plain = np.array(words, dtype=np.uint64)                                  # packed words as a plain array
        dev = torch.from_numpy(plain.view(np.int64).copy()).cuda()
        torch.cuda.synchronize()
        for path in (0, 1, 2):
            _same(_run(g, Q, k, off + np.flatnonzero(mask), path), want, "global ids, path %d" % path)
            _same(_run(g, Q, k, words, path), want, "AllowBits words, path %d" % path)
            _same(_run(g, Q, k, _lib.allow_bitmap(plain, n, packed=True), path), want, "packed words, path %d" % path)
            _same(_run(g, Q, k, None, path, allow_ptr=dev.data_ptr()), want, "device bitmap, path %d" % path)
    finally:
        g.close()


def test_append_invalidates_the_cached_subgallery():
    from isehr_amd import _lib
    rng = np.random.default_rng(99)
    n0, n1, d, k = 600, 630, 32, 6                           # 600 and 630 rows take the same 10 bitmap words
    X = lt.int_rows(rng, n1, d)
    X[:n0, 0] = np.minimum(X[:n0, 0], lt.HI - 1)
    X[n0:, 0] = lt.HI                                        # the appended rows lead query 0
    Q = np.concatenate([np.eye(d, dtype=np.float32)[:3], lt.dense_queries(rng, 4, d)])
    S = lt.int_scores(X, Q)
    m0 = rng.random(n0) < 0.3
    g = _lib.Gallery.empty(n1, d, norm_mode=_lib.NORM_NONE)
    try:
        g.append(X[:n0])
        assert np.array_equal(g.get_rows(0, n0).view(np.uint32), X[:n0].view(np.uint32))
        _same(_run(g, Q, k, m0, 1), lt.filtered_truth(S[:, :n0], m0, k), "before the append")
        assert _run(g, Q, k, m0, 1)[2]["cache_hit"] == 1
        g.append(X[n0:])
        assert np.array_equal(g.get_rows(0, n1).view(np.uint32), X.view(np.uint32))
        same_words = np.concatenate([m0, np.zeros(n1 - n0, bool)])               # the bitmap words of the cached call
        assert np.array_equal(np.asarray(_lib.allow_bitmap(same_words, n1)), np.asarray(_lib.allow_bitmap(m0, n0)))
        idx, sc, info = _run(g, Q, k, same_words, 1)
        assert info["cache_hit"] == 0
        _same((idx, sc), lt.filtered_truth(S, same_words, k), "after the append, the old rows")
        grown = np.concatenate([m0, np.ones(n1 - n0, bool)])
        idx, sc, info = _run(g, Q, k, grown, 1)
        assert info["cache_hit"] == 0 and (idx[0] >= n0).all()
        _same((idx, sc), lt.filtered_truth(S, grown, k), "after the append, the new rows allowed")
        _every_path(g, Q, S, k, grown, "after the append")
    finally:
        g.close()
