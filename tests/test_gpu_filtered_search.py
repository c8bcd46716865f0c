"""GPU: exact filtered top-K (mi_knn_search_filtered, Gallery.search_filtered, KNN.search(allow=...)).

Truth is the float64 score of every stored row (Gallery.get_rows) computed on the host, the disallowed rows set to -inf, judged
by oracle.check_topk_parity; the returned scores must be those float64 values rounded to f32.  Where the comparison must be to
the bit (forced paths against each other and against the unfiltered search), idx and the score bits are compared directly."""
import numpy as np
import pytest

import oracle
from _fullsize import host_f64_scores_and_topk

pytestmark = pytest.mark.gpu

N1, D = 200_000, 2048
TAU = 1e-6           # NORM_L2: f64 (host) vs f32 (device) query normalisation
SELS = ["none", "five", 1e-3, 1e-2, 0.1, 0.5, 0.99]
NQS = [1, 70, 300, 1024, 2500]
KS = [1, 100, 1000]


def _gauss(seed, n, d=D):
    return np.random.default_rng(seed).standard_normal((n, d), dtype=np.float32)


def _mask(sel, n, seed=7):
    rng = np.random.default_rng(seed)
    m = np.zeros(n, bool)
    if sel == "none":
        return m
    if sel == "five":
        m[rng.choice(n, 5, replace=False)] = True
        return m
    m[rng.random(n) < sel] = True
    return m


def _bits_equal(a, b):
    assert (a[0] == b[0]).all()
    assert (a[1].view(np.uint32) == b[1].view(np.uint32)).all()


def check_filtered(idx, sc, S, mask, k, tau=TAU, row_offset=0, rows=None):
    """idx / sc [Q, k]: a filtered answer; S [Q', N] host f64 truth (query i of the answer is row rows[i] of S)."""
    rows = np.arange(idx.shape[0]) if rows is None else rows
    ke = min(k, int(mask.sum()))
    assert (idx[:, ke:] == -1).all() and np.isneginf(sc[:, ke:]).all()
    if ke == 0:
        return
    loc = idx[:, :ke] - row_offset
    assert (loc >= 0).all() and (loc < len(mask)).all()
    assert mask[loc].all(), "a disallowed row was returned"
    Sm = np.where(mask[None, :], S[rows], -np.inf)
    assert oracle.check_topk_parity(loc, Sm, ke, tau) == []
    got = np.take_along_axis(S[rows], loc, 1)
    assert np.abs(got - sc[:, :ke]).max() <= 3e-7 * max(1.0, np.abs(got).max())


@pytest.fixture(scope="module")
def big():
    from isehr_amd import _lib
    X = _gauss(801, N1)
    Q = _gauss(802, 1024)
    g = _lib.Gallery.from_host(X, norm_mode=_lib.NORM_L2)
    S, _, _ = host_f64_scores_and_topk(g, Q, 1)
    yield g, Q, S
    g.set_option("filter_path", 0)
    g.close()


def _run(g, q, k, mask, path):
    g.set_option("filter_path", path)
    try:
        return g.search_filtered(q, k, mask)
    finally:
        g.set_option("filter_path", 0)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("sel", SELS)
def test_answers_paths_and_batches(big, sel, k):
    g, Q, S = big
    mask = _mask(sel, N1)
    rows = np.arange(max(NQS)) % len(Q)
    q = np.ascontiguousarray(Q[rows])
    g.set_option("filter_cache", 0)                          # no sub-gallery, no bitmap remembered from earlier calls
    g.set_option("filter_cache", 1)
    allowed = int(mask.sum())
    cmax = g.get_option("filter_compact_max")
    idx, sc, _, info = _run(g, q, k, mask, 0)
    assert info["allowed"] == allowed
    first = 0 if allowed == 0 else 1 if (allowed / N1 <= cmax or allowed < k) else 2
    assert info["path"] == first
    # the same bitmap again: auto compacts (and keeps the sub-gallery), the call after that reuses it
    i1, s1, _, inf1 = _run(g, q, k, mask, 0)
    _bits_equal((i1, s1), (idx, sc))
    assert inf1["path"] == (0 if allowed == 0 else 1)
    if allowed:
        i1, s1, _, inf1 = _run(g, q, k, mask, 0)
        _bits_equal((i1, s1), (idx, sc))
        assert inf1["path"] == 1 and inf1["cache_hit"] == 1
    pick = np.arange(0, len(rows), 23)                      # every 23rd query against the host truth ...
    check_filtered(idx[pick], sc[pick], S, mask, k, rows=rows[pick])
    for path in (1, 2):                                     # ... and both forced paths to the bit
        i2, s2, _, inf2 = _run(g, q, k, mask, path)
        _bits_equal((i2, s2), (idx, sc))
        if sel != "none":
            assert inf2["path"] == path
    for nq in NQS[:-1]:                                     # any batch size: the same rows
        i3, s3, _, _ = g.search_filtered(Q[:nq], k, mask)
        _bits_equal((i3, s3), (idx[:nq], sc[:nq]))
    if k == 100 and sel in (1e-2, 0.5):
        check_filtered(idx[:300], sc[:300], S, mask, k, rows=rows[:300])


@pytest.mark.parametrize("nq", [300, 1100])
def test_all_rows_allowed_equals_search(big, nq):
    g, Q, _ = big
    q = np.ascontiguousarray(Q[np.arange(nq) % len(Q)])
    ref = g.search(q, 100)[:2]
    ones = np.ones(N1, bool)
    for path in (0, 1, 2):
        i, s, _, info = _run(g, q, 100, ones, path)
        _bits_equal((i, s), ref)
        if path == 2:
            assert info["rerun_queries"] == 0


def test_scores_match_unfiltered_search(big):
    g, Q, _ = big
    full_i, full_s, _ = g.search(Q[:70], 2048)
    for sel in (1e-2, 0.5):
        mask = _mask(sel, N1, seed=11)
        for path in (1, 2):
            i, s, _, _ = _run(g, Q[:70], 1000, mask, path)
            for q in range(70):
                common, a, b = np.intersect1d(i[q], full_i[q], return_indices=True)
                assert len(common) > 0
                assert (s[q][a].view(np.uint32) == full_s[q][b].view(np.uint32)).all()


def test_correlated_filter_reruns():
    """Clustered rows; each query's own cluster is excluded: the over-fetch finds none of its top rows allowed."""
    from isehr_amd import _lib
    d, nc, per = 256, 40, 1000
    rng = np.random.default_rng(901)
    centers = rng.standard_normal((nc, d)).astype(np.float32) * 4
    lab = np.repeat(np.arange(nc), per)
    X = centers[lab] + rng.standard_normal((nc * per, d)).astype(np.float32)
    g = _lib.Gallery.from_host(X, norm_mode=_lib.NORM_L2)
    try:
        R = g.get_rows(0, g.n).astype(np.float64)
        for c in (0, 17, 39):
            q = centers[c] + 0.5 * rng.standard_normal((20, d)).astype(np.float32)
            qn = q.astype(np.float64) / np.linalg.norm(q.astype(np.float64), axis=1)[:, None]
            S = qn @ R.T
            mask = lab != c
            g.set_option("filter_path", 2)
            try:
                idx, sc, _, info = g.search_filtered(q, 50, mask)
            finally:
                g.set_option("filter_path", 0)
            assert info["path"] == 2 and info["rerun_queries"] > 0
            check_filtered(idx, sc, S, mask, 50)
            i0, s0, _, _ = g.search_filtered(q, 50, mask)              # auto: the same answer
            _bits_equal((i0, s0), (idx, sc))
    finally:
        g.close()


def test_cache_append_and_image_type():
    from isehr_amd import _lib
    d, n0, n1 = 512, 30_000, 34_000
    X = _gauss(1001, n1, d)
    Q = _gauss(1002, 40, d)
    g = _lib.Gallery.empty(n1, d)
    try:
        g.append(X[:n0])
        g.set_option("filter_path", 1)
        m0 = _mask(0.05, n0, seed=3)
        a, b, _, i1 = g.search_filtered(Q, 20, m0)
        assert i1["cache_hit"] == 0
        a2, b2, _, i2 = g.search_filtered(Q, 20, m0)
        assert i2["cache_hit"] == 1
        _bits_equal((a2, b2), (a, b))
        m1 = _mask(0.05, n0, seed=4)
        _, _, _, i3 = g.search_filtered(Q, 20, m1)
        assert i3["cache_hit"] == 0
        _, _, _, i4 = g.search_filtered(Q, 20, m1)
        assert i4["cache_hit"] == 1
        # append: the stored sub-gallery is stale; the new rows are found when allowed
        g.append(X[n0:])
        m2 = np.concatenate([m1, np.ones(n1 - n0, bool)])
        idx, sc, _, i5 = g.search_filtered(Q, 20, m2)
        assert i5["cache_hit"] == 0
        R = g.get_rows(0, n1).astype(np.float64)
        S = (Q.astype(np.float64) / np.linalg.norm(Q.astype(np.float64), axis=1)[:, None]) @ R.T
        check_filtered(idx, sc, S, m2, 20)
        assert (idx >= n0).any()
        m1x = np.concatenate([m1, np.zeros(n1 - n0, bool)])
        _, _, _, i6 = g.search_filtered(Q, 20, m1x)
        assert i6["cache_hit"] == 0
        # image type change: rebuilt, same answer (the scores come from the f32 rows)
        ref = g.search_filtered(Q, 20, m2)
        g.set_image_dtype(0)
        got = g.search_filtered(Q, 20, m2)
        assert got[3]["cache_hit"] == 0
        _bits_equal(got[:2], ref[:2])
        # filter_cache 0: never reused
        g.set_option("filter_cache", 0)
        assert g.search_filtered(Q, 20, m2)[3]["cache_hit"] == 0
        assert g.search_filtered(Q, 20, m2)[3]["cache_hit"] == 0
    finally:
        g.close()


def test_row_offset_and_device_bitmap():
    import torch
    from isehr_amd import _lib
    n, d, off = 20_000, 384, 5_000_000
    X = _gauss(1101, n, d)
    Q = _gauss(1102, 30, d)
    g = _lib.Gallery.from_host(X, norm_mode=_lib.NORM_L2, row_offset=off)
    try:
        ids = off + np.random.default_rng(5).choice(n, 3000, replace=False)
        mask = np.zeros(n, bool)
        mask[ids - off] = True
        R = g.get_rows(0, n).astype(np.float64)
        S = (Q.astype(np.float64) / np.linalg.norm(Q.astype(np.float64), axis=1)[:, None]) @ R.T
        for path in (1, 2):
            g.set_option("filter_path", path)
            idx, sc, _, _ = g.search_filtered(Q, 25, ids)
            check_filtered(idx, sc, S, mask, 25, row_offset=off)
            words = _lib.allow_bitmap(ids, n, off)
            dev = torch.from_numpy(np.asarray(words).view(np.int64).copy()).cuda()
            torch.cuda.synchronize()
            i2, s2, _, _ = g.search_filtered(Q, 25, allow_ptr=dev.data_ptr())
            _bits_equal((i2, s2), (idx, sc))
        g.set_option("filter_path", 0)
    finally:
        g.close()


def test_no_interference(big):
    import torch
    g, Q, S = big
    ref = g.search(Q[:300], 100)[:2]
    ref_small = g.search(Q[:50], 100)[:2]
    mask = np.ones(N1, bool)
    mask[np.argsort(-S[:300], axis=1)[:, :100].ravel()] = False  # the queries' own best rows: the over-fetch re-runs them
    assert g.flags() == 0
    for _ in range(2):
        g.set_option("filter_path", 2)
        try:
            _, _, _, info = g.search_filtered(Q[:300], 100, mask)
        finally:
            g.set_option("filter_path", 0)
        assert info["rerun_queries"] > 0
        assert g.flags() == 0
        _bits_equal(g.search(Q[:300], 100)[:2], ref)
        g.search_filtered(Q[:1], 10, _mask(1e-3, N1))
        _bits_equal(g.search(Q[:50], 100)[:2], ref_small)
    # a deferred tail (async_tail 3) pending from search_device when the filtered search starts
    k, nq = 100, 512
    q = torch.from_numpy(Q[:nq]).cuda()
    want = g.search(Q[:nq], k)[0]
    fref = g.search_filtered(Q[:129], 50, mask)
    ix = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    g.set_option("async_tail", 3)
    try:
        torch.cuda.synchronize()
        g.search_device(q.data_ptr(), nq, k, ix.data_ptr())       # its tail is deferred to the next call
        mid = g.search_filtered(Q[:129], 50, mask)
        g.join()
        torch.cuda.synchronize()
    finally:
        g.set_option("async_tail", 0)
    assert (ix.cpu().numpy() == want).all()
    _bits_equal(mid[:2], fref[:2])
    _bits_equal(g.search(Q[:300], 100)[:2], ref)


def test_norm_none_f32_scorer_route():
    """Raw rows of heavy-tailed norms (fp16 image) and queries whose fp16 image overflows: the batch goes to the f32 scorer."""
    from isehr_amd import _lib
    n, d = 40_000, 512
    rng = np.random.default_rng(1201)
    X = rng.standard_normal((n, d)).astype(np.float32)
    norms = np.minimum(3.5, 0.05 * (1 + rng.pareto(1.5, n)))
    X *= (norms / np.linalg.norm(X, axis=1))[:, None].astype(np.float32)
    Q = rng.standard_normal((24, d)).astype(np.float32)
    Q[:, 0] = 1e5                                            # beyond fp16's range
    g = _lib.Gallery.from_host(X, norm_mode=_lib.NORM_NONE)
    try:
        R = g.get_rows(0, n).astype(np.float64)
        S = Q.astype(np.float64) @ R.T
        before = g.status()["overflow_batches"]
        g.search(Q, 10)
        assert g.status()["overflow_batches"] > before          # the unfiltered search takes the f32 route on these queries
        tau = 1e-9 * np.abs(S).max()
        for sel in (0.01, 0.6):
            mask = _mask(sel, n, seed=13)
            for path in (1, 2):
                g.set_option("filter_path", path)
                idx, sc, _, _ = g.search_filtered(Q, 10, mask)
                check_filtered(idx, sc, S, mask, 10, tau=tau)
        g.set_option("filter_path", 0)
        # a sticky flag left by the asynchronous device entry point (FLAG_RANGE: these queries' fp16 image overflows) is
        # still there, unchanged, after a filtered call on either path -- one that raised and cleared its own flags inside
        import torch
        qd = torch.from_numpy(Q).cuda()
        ix = torch.empty((len(Q), 10), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        g.search_device(qd.data_ptr(), len(Q), 10, ix.data_ptr())
        want = g.flags()
        assert want & 8
        for path in (1, 2):
            g.search_device(qd.data_ptr(), len(Q), 10, ix.data_ptr())
            g.set_option("filter_path", path)
            g.search_filtered(Q, 10, _mask(0.6, n, seed=13))
            g.set_option("filter_path", 0)
            assert g.flags() == want
        assert g.flags() == 0
    finally:
        g.close()


def test_knn_wrapper():
    from isehr_amd import _lib
    from isehr_amd.knn import KNN
    X = _gauss(1301, 5000, 256)
    Q = _gauss(1302, 8, 256)
    knn = KNN(X)
    try:
        S = Q.astype(np.float64) @ X.astype(np.float64).T
        allow = np.arange(100, 5000, 7)
        mask = np.zeros(5000, bool)
        mask[allow] = True
        Dv, Iv = knn.search(Q, 12, allow=allow)
        assert Dv.shape == (8, 12) and Iv.shape == (8, 12) and Dv.dtype == np.float32 and Iv.dtype == np.int64
        check_filtered(Iv, Dv, S, mask, 12, tau=1e-9)
        Dp, Ip = knn.search(Q, 12, allow=np.array([3, 4000]))      # fewer allowed rows than k: -1 padding
        assert (Ip[:, 2:] == -1).all() and np.isneginf(Dp[:, 2:]).all()
        assert set(Ip[0, :2].tolist()) == {3, 4000}
        Dr, Ir = knn.search(Q, 12, allow=_lib.allow_ranges([(0, 1000), (4000, 5000)], 5000))
        rm = np.zeros(5000, bool)
        rm[:1000] = rm[4000:] = True
        check_filtered(Ir, Dr, S, rm, 12, tau=1e-9)
    finally:
        knn.close()


@pytest.mark.parametrize("sel", [0.01, 0.5])
def test_full_size(sel):
    import torch
    from isehr_amd import _lib
    from isehr_amd.synth import synth_rows
    N = 1005994
    s = torch.cuda.current_stream().cuda_stream
    raw = torch.empty((N, D), dtype=torch.float32, device="cuda")
    _lib.synth_fill_device(raw.data_ptr(), 4321, 0, N, D, s)
    torch.cuda.synchronize()
    g = _lib.Gallery.from_device_ptr(raw.data_ptr(), N, D)
    del raw
    try:
        Q = synth_rows(4322, 0, 64, D)
        S, _, _ = host_f64_scores_and_topk(g, Q, 1)
        mask = _mask(sel, N, seed=17)
        idx, sc, _, info = g.search_filtered(Q, 100, mask)
        assert info["allowed"] == mask.sum()
        check_filtered(idx, sc, S, mask, 100)
    finally:
        g.close()
