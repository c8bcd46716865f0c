"""GPU: exact grouped top-K (mi_knn_search_grouped, csrc/api_group.hip, csrc/group_select.hip) against the
sequential walk of tests/_grouped_truth.py over two independent complete rankings: the library's own (Gallery.search at depth n,
Gallery.rank_all above 2048 rows) and numpy's on the integer lattice of tests/_lattice_truth.py, where every score is exact.  Every
case runs on "group_path" 0, 1 and 2; the three must agree on ids, score bits and labels and equal the truths.

Above 2048 rows the library's ranking is rank_all's, whose float32 scores are the search's bits only on exact data: those cases
use the lattice.  The d = 2048 case has Gaussian rows (the lattice ends at d = 128) and the library's ranking alone."""
import numpy as np
import pytest

import _grouped_truth as gt
import _lattice_truth as lt

pytestmark = pytest.mark.gpu


def _same(got, want, what=""):
    ig, sg, lg = got
    iw, sw, lw = want
    assert ig.dtype == np.int64 and sg.dtype == np.float32 and lg.dtype == np.int32
    assert ig.shape == iw.shape and sg.shape == sw.shape and lg.shape == lw.shape
    if not np.array_equal(ig, iw):
        q, j = (int(v[0]) for v in np.nonzero(ig != iw))
        raise AssertionError("%s: query %d, position %d: row %d (score %r), the truth has row %d (score %r)"
                             % (what, q, j, ig[q, j], sg[q, j], iw[q, j], sw[q, j]))
    assert np.array_equal(sg.view(np.uint32), sw.view(np.uint32)), "%s: score bits differ" % what
    assert np.array_equal(lg, lw), "%s: labels differ" % what


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


def _run(g, Q, k, exclude=None, path=0):
    g.set_option("group_path", path)
    try:
        idx, sc, _, lab, info = g.search_grouped(Q, k, exclude, return_labels=True, return_info=True)
    finally:
        g.set_option("group_path", 0)
    return (idx, sc, lab), info


def _kprime(g, k):
    from isehr_amd import _lib
    f = int(_lib.get_global_option("group_overfetch"))
    return min(2048, g.n, f * k + 32)


def _every_path(g, Q, ks, labels, rankings, exclude=None, what=""):
    """k (or every k of a list) on paths 0, 1 and 2 against the walk over every ranking of `rankings` -> the three infos of the
    last k.  The walk to the largest k is made once: the walk to a smaller k is its first k columns."""
    ks = [ks] if np.isscalar(ks) else list(ks)
    deep = [gt.grouped_truth(ids, sc, labels, max(ks), exclude, g.row_offset) for ids, sc in rankings]
    for k in ks:
        wants = [tuple(a[:, :k] for a in w) for w in deep]
        for w in wants[1:]:
            _same(w, wants[0], "%s, k %d: the two truths" % (what, k))
        infos = []
        for path in (0, 1, 2):
            got, info = _run(g, Q, k, exclude, path)
            _same(got, wants[0], "%s, k %d, path %d" % (what, k, path))
            assert info["path"] == (1 if path == 1 else 2) and info["kprime"] == (0 if path == 1 else _kprime(g, k))
            assert info["groups"] == g.group_count()
            infos.append(info)
    return infos


@pytest.mark.parametrize("n, d, nq", [(1, 64, 1), (63, 64, 70), (65, 64, 1), (300, 64, 70), (2049, 64, 70), (4100, 64, 1),
                                      (300, 2048, 70)])
def test_shapes(n, d, nq):
    """cases 1, 2 and the random labels of every shape: all labels -1 is Gallery.search bit for bit, one group is one row and
    padding, random groups of 1 .. 7 rows with a random excluded label per query"""
    rng = np.random.default_rng(100 * n + d)
    if d <= lt.D_MAX:
        X, Q = lt.int_rows(rng, n, d), lt.dense_queries(rng, nq, d)
    else:
        X, Q = rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((nq, d)).astype(np.float32)
    ks = [k for k in (1, 10, 100, 2048) if k <= n]
    g = _gallery(X)
    try:
        rankings = [gt.library_ranking(g, Q)] + ([gt.lattice_ranking(X, Q)] if d <= lt.D_MAX else [])
        single = np.full(n, -1, np.int32)
        g.set_groups(single)
        assert g.group_count() == n
        for k in ks:
            infos = _every_path(g, Q, k, single, rankings, what="n %d, all -1" % n)
            assert infos[0]["rerun_queries"] == 0 and infos[2]["rerun_queries"] == 0
            ref = g.search(Q, k)[:2]
            for path in (0, 1, 2):
                got = _run(g, Q, k, None, path)[0]
                _same(got, (ref[0], ref[1], np.full((nq, k), -1, np.int32)), "n %d, all -1 against search, path %d" % (n, path))
        one = np.full(n, 5, np.int32)
        g.set_groups(one)
        assert g.group_count() == 1
        for k in ks:
            _every_path(g, Q, k, one, rankings, what="n %d, one group" % n)
            (idx, sc, lab), _ = _run(g, Q, k)
            assert (idx[:, 0] == rankings[0][0][:, 0]).all() and (lab[:, 0] == 5).all()
            assert (idx[:, 1:] == -1).all() and np.isneginf(sc[:, 1:]).all() and (lab[:, 1:] == -1).all()
        labels = gt.random_labels(rng, n, spread=3)
        g.set_groups(labels)
        assert g.group_count() == len(set(labels[labels >= 0].tolist())) + int((labels < 0).sum())
        exclude = labels[rng.integers(0, n, nq)]
        _every_path(g, Q, ks, labels, rankings, what="n %d, random groups" % n)
        _every_path(g, Q, ks, labels, rankings, exclude, what="n %d, random groups, exclusion" % n)
    finally:
        g.close()


def _giant(rng, n, d, planted):
    """rows `A` (planted of them, at random places) score 6 .. 12 against every query, the others at most 3: column 0 is 3 on A
    (planted_gallery) and <= 0 elsewhere, a query is 3 e_0 +- e_c"""
    X, _ = lt.planted_gallery(rng, n, d, 3, [(planted, planted)])
    A = X[:, 0] == 3
    assert A.sum() == planted
    X[~A, 0] = np.minimum(X[~A, 0], 0)
    return X, A


@pytest.mark.parametrize("nq", [1, 70])
def test_giant_group(nq):
    """case 3: 3000 of 4100 rows share one label and lead every query's ranking, so the top 2048 hold one group: a forced
    over-fetch certifies nothing and the dense fallback answers every query"""
    rng = np.random.default_rng(4100 + nq)
    n, d, k = 4100, 64, 10
    X, A = _giant(rng, n, d, 3000)
    Q = np.zeros((nq, d), np.float32)
    Q[:, 0] = 3
    Q[np.arange(nq), 1 + np.arange(nq) % (d - 1)] = np.where(np.arange(nq) < d - 1, 1, -1)
    labels = gt.random_labels(rng, n, singles=0.1)
    labels[A] = 10 ** 6
    g = _gallery(X)
    try:
        g.set_groups(labels)
        rankings = [gt.library_ranking(g, Q), gt.lattice_ranking(X, Q)]
        # the premise, from the host ranking: the top 2048 rows of every query hold fewer than k groups (here: one)
        top = labels[rankings[1][0][:, :2048]]
        assert all(len(set(row.tolist())) < k for row in top) and (top == 10 ** 6).all()
        from isehr_amd import _lib
        # at the default factor (K' = 4 k + 32 = 72) and at the deepest list there is ("group_overfetch" 2048: K' = 2048)
        for f, kp in ((0, 72), (2048, 2048)):
            _lib.set_global_option("group_overfetch", f)
            try:
                infos = _every_path(g, Q, k, labels, rankings, what="giant group, nq %d, K' %d" % (nq, kp))
            finally:
                _lib.set_global_option("group_overfetch", 0)
            assert infos[2]["rerun_queries"] == nq and infos[2]["kprime"] == kp
            assert infos[0]["rerun_queries"] == nq and infos[1]["rerun_queries"] == 0
        # the giant group excluded: the fallback again (K' rows of an excluded group certify nothing), and it is gone
        ex = np.full(nq, 10 ** 6)
        infos = _every_path(g, Q, k, labels, rankings, ex, what="giant group excluded, nq %d" % nq)
        assert infos[2]["rerun_queries"] == nq and infos[2]["excluded_found"] == nq
        assert (_run(g, Q, k, ex)[0][2] != 10 ** 6).all()
        # sub-batches of one query ("group_dense_bytes" below one query's scores): the same answer
        _lib.set_global_option("group_dense_bytes", 1)
        try:
            _every_path(g, Q, k, labels, rankings, what="giant group, one query per sub-batch")
        finally:
            _lib.set_global_option("group_dense_bytes", 0)
    finally:
        g.close()


def test_ties():
    """case 4 on lattice data: identical rows in two groups (the lower id's group first), identical rows inside a group (the
    lowest id is reported), tie classes that straddle rank k (one-hot queries: seven score levels over 300 rows)"""
    rng = np.random.default_rng(44)
    n, d = 300, 64
    X = lt.int_rows(rng, n, d)
    Q = np.concatenate([lt.dense_queries(rng, 2, d), np.eye(d, dtype=np.float32)[:6] * np.float32(2)])
    best = lambda q: (lt.HI * np.sign(q)).astype(np.float32)     # noqa: E731  the lattice row that scores highest against q
    X[7] = X[10] = best(Q[0])
    X[20] = X[21] = X[22] = best(Q[1])
    labels = gt.random_labels(rng, n)
    labels[labels >= 0] += 1000
    labels[[5, 10]] = 1                                          # group A
    labels[7] = 2                                                # group B
    labels[[20, 21, 22]] = 3
    g = _gallery(X)
    try:
        g.set_groups(labels)
        rankings = [gt.library_ranking(g, Q), gt.lattice_ranking(X, Q)]
        S = lt.int_scores(X, Q)
        assert S[0, 7] == S[0, 10] == S[0].max() and (S[0] == S[0].max()).sum() == 2
        assert S[1, 20] == S[1].max() and (S[1] == S[1].max()).sum() == 3
        _every_path(g, Q, (1, 2, 10, 100), labels, rankings, what="ties")
        for path in (1, 2):
            (idx, sc, lab), _ = _run(g, Q, 10, None, path)
            assert idx[0, :2].tolist() == [7, 10] and lab[0, :2].tolist() == [2, 1]       # B (row 7) before A (row 10, not 5)
            assert idx[1, 0] == 20 and lab[1, 0] == 3 and 21 not in idx[1] and 22 not in idx[1]
        # the one-hot queries: the score at rank k is shared by rows on both sides of the cut
        want = gt.grouped_truth(*rankings[1], labels, 10)
        full = gt.grouped_truth(*rankings[1], labels, n)
        assert all((full[1][q] == want[1][q, -1]).sum() > (want[1][q] == want[1][q, -1]).sum() for q in range(2, 8))
    finally:
        g.close()


def test_exclusion():
    """case 5"""
    rng = np.random.default_rng(55)
    n, d, nq, k = 300, 64, 70, 10
    X, Q = lt.int_rows(rng, n, d), lt.dense_queries(rng, nq, d)
    labels = gt.random_labels(rng, n, singles=0.0)
    g = _gallery(X)
    try:
        g.set_groups(labels)
        rankings = [gt.library_ranking(g, Q), gt.lattice_ranking(X, Q)]
        own = labels[rankings[1][0][:, 0]]                       # every query's best group
        infos = _every_path(g, Q, k, labels, rankings, own, what="own group excluded")
        assert all(i["excluded_found"] == nq for i in infos)
        (idx, sc, lab), _ = _run(g, Q, k, own)
        assert (lab != own[:, None]).all()
        plain = _run(g, Q, k)[0]
        assert (plain[2][:, 0] == own).all() and not np.array_equal(plain[0], idx)
        for name, ex in (("a label no row carries", np.full(nq, 2 ** 30)), ("-1", np.full(nq, -1)), ("one label for all", -1)):
            for path in (0, 1, 2):
                got, info = _run(g, Q, k, ex, path)
                _same(got, plain, "exclude %s, path %d" % (name, path))
                assert info["excluded_found"] == 0
        mixed = np.where(np.arange(nq) % 2 == 0, own, 2 ** 30)
        assert _every_path(g, Q, k, labels, rankings, mixed, what="every other query excludes")[0]["excluded_found"] == (nq + 1) // 2
        few = (np.arange(n) % 3).astype(np.int32) * 7            # three groups, one excluded: two results, then padding
        g.set_groups(few)
        _every_path(g, Q, 5, few, rankings, np.full(nq, 7), what="fewer than k groups left")
        (idx, sc, lab), _ = _run(g, Q, 5, np.full(nq, 7))
        assert (idx[:, :2] >= 0).all() and (idx[:, 2:] == -1).all() and np.isneginf(sc[:, 2:]).all() and (lab[:, 2:] == -1).all()
        assert set(lab[:, :2].ravel().tolist()) == {0, 14}
    finally:
        g.close()


def test_labels():
    """case 6: labels that are not dense, up to 2**31 - 1, mixed with -1"""
    rng = np.random.default_rng(66)
    n, d, nq, k = 300, 64, 9, 100
    X, Q = lt.int_rows(rng, n, d), lt.dense_queries(rng, nq, d)
    pool = np.array([0, 3, 17, 2 ** 20 + 1, 2 ** 31 - 2, 2 ** 31 - 1], np.int64)
    labels = pool[rng.integers(0, len(pool), n)]
    labels[rng.random(n) < 0.5] = -1
    labels[:6] = pool
    labels = labels.astype(np.int32)
    g = _gallery(X)
    try:
        g.set_groups(labels)
        assert np.array_equal(g.groups(), labels) and g.groups().dtype == np.int32
        assert g.group_count() == len(pool) + int((labels < 0).sum())
        rankings = [gt.library_ranking(g, Q), gt.lattice_ranking(X, Q)]
        _every_path(g, Q, k, labels, rankings, what="labels")
        (idx, sc, lab), _ = _run(g, Q, k)
        assert np.array_equal(lab, labels[idx]) and 2 ** 31 - 1 in lab
        _every_path(g, Q, k, labels, rankings, np.full(nq, 2 ** 31 - 1), what="labels, 2**31 - 1 excluded")
        g.set_groups(labels.astype(np.int64))                    # any integer dtype
        assert np.array_equal(g.groups(), labels)
    finally:
        g.close()


def test_offsets_layouts_and_depths():
    """case 7: row_offset, f64 and strided queries, and the two edges of the collapse kernel's list length"""
    from isehr_amd import _lib
    rng = np.random.default_rng(77)
    n, d, nq, off = 2049, 64, 70, 10 ** 6
    X, Q = lt.int_rows(rng, n, d), lt.dense_queries(rng, nq, d)
    labels = gt.random_labels(rng, n, max_size=2)
    g = _gallery(X, row_offset=off)
    try:
        g.set_groups(labels)
        rankings = [gt.library_ranking(g, Q), gt.lattice_ranking(X, Q, off)]
        assert rankings[0][0].min() == off
        for k in (10, 504, 600):                                 # 4 k + 32: 72, 2048 exactly, beyond 2048
            infos = _every_path(g, Q, k, labels, rankings, what="row_offset 10**6")
            assert infos[2]["kprime"] == min(2048, 4 * k + 32)
        assert _lib.get_global_option("group_overfetch") == 4 and _kprime(g, 504) == 2048
        want = _run(g, Q, 10)[0]
        assert want[0].min() >= off
        QT = np.asfortranarray(Q)                                # the reference's [D, Q] array, transposed: column stride Q
        assert not QT.flags.c_contiguous
        for path in (0, 1, 2):
            _same(_run(g, Q.astype(np.float64), 10, None, path)[0], want, "f64 queries, path %d" % path)
            _same(_run(g, QT, 10, None, path)[0], want, "strided queries, path %d" % path)
            _same(_run(g, np.asfortranarray(Q.astype(np.float64)), 10, None, path)[0], want, "strided f64 queries, path %d" % path)
    finally:
        g.close()
    # K' = n < f k + 32: the list covers the shard, every query is certified whatever it kept
    n = 63
    X = lt.int_rows(rng, n, d)
    labels = (np.arange(n) % 4).astype(np.int32)
    g = _gallery(X)
    try:
        g.set_groups(labels)
        rankings = [gt.library_ranking(g, Q), gt.lattice_ranking(X, Q)]
        infos = _every_path(g, Q, 10, labels, rankings, what="K' = n")
        assert infos[2]["kprime"] == n and infos[2]["rerun_queries"] == 0
    finally:
        g.close()


def test_state():
    """case 8"""
    import torch
    from isehr_amd import _lib
    rng = np.random.default_rng(88)
    n, d, nq, k = 300, 64, 5, 10
    X, Q = lt.int_rows(rng, n + 40, d), lt.dense_queries(rng, nq, d)
    labels = gt.random_labels(rng, n + 40)
    g = _lib.Gallery.empty(n + 40, d, norm_mode=_lib.NORM_NONE)
    try:
        g.append(X[:n])
        for call in (lambda: g.search_grouped(Q, k), g.groups, g.group_count):
            with pytest.raises(RuntimeError, match="error 1: .*in step"):
                call()
        for bad in (labels[:n - 1], labels[:n + 1]):
            with pytest.raises(RuntimeError, match="error 1: "):
                g.set_groups(bad)
        wrong = labels[:n].copy()
        wrong[17] = -2
        with pytest.raises(RuntimeError, match="error 1: "):
            g.set_groups(wrong)
        with pytest.raises(RuntimeError, match="in step"):       # a refused call sets nothing
            g.group_count()
        g.set_groups(labels[:n])
        rank = lambda m: [gt.library_ranking(g, Q), gt.lattice_ranking(X[:m], Q)]     # noqa: E731
        _every_path(g, Q, k, labels[:n], rank(n), what="before the append")
        for bad_k in (0, 2049):
            with pytest.raises(RuntimeError, match="error 1: "):
                g.search_grouped(Q, bad_k)
        g.append(X[n:])
        with pytest.raises(RuntimeError, match="error 1: .*in step"):
            g.search_grouped(Q, k)
        g.set_groups(labels)
        _every_path(g, Q, k, labels, rank(n + 40), what="after the append")
        kept = g.remove(np.arange(n + 40) % 5 == 0)
        with pytest.raises(RuntimeError, match="error 1: .*in step"):
            g.search_grouped(Q, k)
        g.set_groups(labels[kept])
        _every_path(g, Q, k, labels[kept], [gt.library_ranking(g, Q), gt.lattice_ranking(X[kept], Q)], what="after the removal")
        g.set_groups(None)
        with pytest.raises(RuntimeError, match="error 1: .*in step"):
            g.search_grouped(Q, k)
    finally:
        g.close()
    # a sticky flag left by the asynchronous device entry point (FLAG_RANGE: these queries' fp16 image overflows) is still there,
    # unchanged, after a grouped call on either path
    R = (0.1 * rng.standard_normal((n, d))).astype(np.float32)
    g = _lib.Gallery.from_host(R, norm_mode=_lib.NORM_NONE)
    try:
        g.set_groups(labels[:n])
        big = Q.copy()
        big[:, 0] = 1e5
        qd = torch.from_numpy(big).cuda()
        ix = torch.empty((nq, k), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        g.search_device(qd.data_ptr(), nq, k, ix.data_ptr())
        want = g.flags()
        assert want & 8
        for path in (1, 2):
            g.search_device(qd.data_ptr(), nq, k, ix.data_ptr())
            _run(g, Q, k, None, path)
            assert g.flags() == want
        assert g.flags() == 0
    finally:
        g.close()
    g = _lib.Gallery.l2_from_host(X)
    try:
        with pytest.raises(RuntimeError, match="error 6: "):
            g.set_groups(labels)
        with pytest.raises(RuntimeError, match="error 6: "):
            g.search_grouped(Q, k)
    finally:
        g.close()


def test_knn_wrapper():
    from isehr_amd.knn import KNN
    rng = np.random.default_rng(99)
    n, d, nq, k = 300, 64, 7, 10
    X, Q = lt.int_rows(rng, n, d), lt.dense_queries(rng, nq, d)
    labels = gt.random_labels(rng, n)
    index = KNN(X, "cosine")
    try:
        index.set_groups(labels)
        ex = labels[:nq]
        sims, ids = index.search_grouped(Q, k, exclude=ex)
        want = gt.grouped_truth(*gt.lattice_ranking(X, Q), labels, k, ex)
        assert np.array_equal(ids, want[0]) and np.array_equal(sims.view(np.uint32), want[1].view(np.uint32))
        full_sims, full_ids = index.search(Q, k)
        assert full_sims.shape == sims.shape and full_ids.dtype == ids.dtype
    finally:
        index.close()
    index = KNN(X, "euclidean")
    try:
        with pytest.raises(NotImplementedError):
            index.set_groups(labels)
    finally:
        index.close()
