"""GPU: exact range search (mi_range_search, Gallery.range_search, KNN.range_search, near_duplicate_pairs).

Truth is the float64 score of every stored row (Gallery.get_rows) computed on the host.  On NORM_NONE galleries the queries
are used as given, so host and device score the same f32 vectors and "exact" means: the same members as `scores >= tau`
except rows within 1e-12 of tau (a host and a device f64 sum may round apart in the last bit).  On NORM_L2 galleries the
device normalises the queries in f32 and the host in f64, which moves a score by up to a few 1e-8: rows within BAND of tau
may go either way there.  Where the comparison must be to the bit (agreement with top-K), tau is the device's own f64 score
of the K-th row (mi_knn_search_device's score64 output)."""
import ctypes as C

import numpy as np
import pytest

from _fullsize import host_f64_scores_and_topk

pytestmark = pytest.mark.gpu

N1, D = 200_000, 2048
BAND = 1e-6          # NORM_L2: f64 (host) vs f32 (device) query normalisation
EXACT = 1e-12        # NORM_NONE: host vs device f64 summation order


def _gauss(seed, n, d=D, dtype=np.float32):
    return np.random.default_rng(seed).standard_normal((n, d), dtype=np.float32).astype(dtype, copy=False)


def check_range(lims, idx, sc, S, tau, band, row_offset=0):
    """lims / idx / sc: one range_search answer; S [Q, N] host f64 truth of the stored rows."""
    nq = S.shape[0]
    band = band * max(1.0, abs(tau))                  # the bands are relative to the scores' scale
    assert lims.shape == (nq + 1,) and lims[0] == 0
    assert (np.diff(lims) >= 0).all()
    assert lims[-1] == len(idx) == len(sc)
    for i in range(nq):
        ids = idx[lims[i]:lims[i + 1]] - row_offset
        s = sc[lims[i]:lims[i + 1]]
        row = S[i]
        want = row >= tau
        amb = np.abs(row - tau) <= band
        got = np.zeros(len(row), bool)
        assert len(np.unique(ids)) == len(ids), "query %d: duplicate ids" % i
        assert ids.min(initial=0) >= 0 and ids.max(initial=0) < len(row)
        got[ids] = True
        bad = (got != want) & ~amb
        assert not bad.any(), "query %d: %d rows differ from scores >= tau (e.g. %s)" % (i, bad.sum(), np.flatnonzero(bad)[:5])
        if len(ids):
            t = row[ids]
            assert (np.abs(t - s) <= 3e-7 * np.maximum(1.0, np.abs(t))).all()
            # order: (score desc, id asc), near-ties may swap
            dt = np.diff(t)
            assert (dt <= 2 * band).all(), "query %d: not in descending score order" % i
            tie = (np.abs(dt) <= band) & (np.diff(s) == 0)
            assert (np.diff(ids)[tie & (dt == 0)] > 0).all()
            assert (np.diff(s) <= 0).all()


def tau_for_hits(S, h):
    """a threshold with about h hits per query: the median over queries of the h-th largest score"""
    kth = -np.partition(-S, h - 1, axis=1)[:, h - 1]
    return float(np.median(kth))


@pytest.fixture(scope="module")
def big():
    from isehr_amd import _lib
    X = _gauss(101, N1)
    Q = _gauss(102, 1024)
    g = _lib.Gallery.from_host(X, norm_mode=_lib.NORM_L2)
    S, _, _ = host_f64_scores_and_topk(g, Q, 1)
    yield g, Q, S
    g.close()


@pytest.mark.parametrize("nq", [1, 70, 128, 129, 257, 1024])
def test_levels(big, nq):
    g, Q, S = big
    Ss = S[:nq]
    taus = [float(S.max()) + 0.01, tau_for_hits(S, 5), tau_for_hits(S, 100), tau_for_hits(S, 3000)]
    for tau in taus:
        lims, idx, sc, _ = g.range_search(Q[:nq], tau)
        check_range(lims, idx, sc, Ss, tau, BAND)
    lims, idx, _, _ = g.range_search(Q[:nq], taus[0])
    assert lims[-1] == 0 and len(idx) == 0


def test_agreement_with_topk(big):
    import torch
    g, Q, S = big
    k, nq = 100, 24
    q = torch.from_numpy(Q[:nq]).cuda()
    ix = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    s64 = torch.empty((nq, k), dtype=torch.float64, device="cuda")
    g.search_device(q.data_ptr(), nq, k, ix.data_ptr(), None, s64.data_ptr())
    g.join()
    torch.cuda.synchronize()
    ix, s64 = ix.cpu().numpy(), s64.cpu().numpy()
    host_idx, _, _ = g.search(Q[:nq], k)
    assert (host_idx == ix).all()
    for i in range(nq):
        tau = float(s64[i, k - 1])          # the device's own f64 score of the K-th row
        lims, idx, sc, _ = g.range_search(Q[i:i + 1], tau)
        got = set(idx.tolist())
        assert set(ix[i].tolist()) <= got
        extra = got - set(ix[i].tolist())
        for e in extra:                     # only rows tied with the K-th score
            assert abs(S[i, e] - S[i, ix[i, k - 1]]) <= BAND
        assert (idx[:k] == ix[i]).all() or extra


def test_near_duplicate_clusters():
    """exact and 1e-4-jittered copies of one row, tau inside the cluster: thousands of rows within eps of tau"""
    from isehr_amd import _lib
    n = 60_000
    X = _gauss(201, n)
    rng = np.random.default_rng(202)
    v = X[7].copy()
    pos = rng.choice(np.arange(100, n), 6000, replace=False)
    X[pos[:2000]] = v
    X[pos[2000:]] = v + 1e-4 * rng.standard_normal((4000, D), dtype=np.float32)
    g = _lib.Gallery.from_host(X, norm_mode=_lib.NORM_L2)
    try:
        Q = np.stack([v, X[pos[2500]], _gauss(203, 1)[0]])
        S, _, _ = host_f64_scores_and_topk(g, Q, 1)
        jit = np.sort(S[0, pos[2000:]])
        for tau in (float(jit[len(jit) // 2]), float(jit[10]), float(jit[-10])):
            lims, idx, sc, _ = g.range_search(Q, tau)
            check_range(lims, idx, sc, S, tau, BAND)
            assert lims[1] - lims[0] > 2000
    finally:
        g.close()


def test_everything_at_tau_minus_one_takes_the_dense_path():
    from isehr_amd import _lib
    n, nq = 20_000, 300
    g = _lib.Gallery.from_host(_gauss(301, n), norm_mode=_lib.NORM_L2)
    try:
        Q = _gauss(302, nq)
        S, _, _ = host_f64_scores_and_topk(g, Q, 1)
        before = g.status()["overflow_batches"]
        lims, idx, sc, _ = g.range_search(Q, -1.0)
        assert g.status()["overflow_batches"] > before
        assert (np.diff(lims) == n).all()
        check_range(lims, idx, sc, S, -1.0, BAND)
        for i in (0, 150, nq - 1):
            row = idx[lims[i]:lims[i + 1]]
            want = np.lexsort((np.arange(n), -S[i]))      # host order; near-ties may swap
            assert (np.abs(S[i][row] - S[i][want]) <= BAND).all()
    finally:
        g.close()


def _answer(g, Q, tau):
    lims, idx, sc, _ = g.range_search(Q, tau)
    return lims, idx, sc


def _same(a, b):
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and (a[2].view(np.uint32) == b[2].view(np.uint32)).all()


def test_paths_give_the_same_answers(big):
    g, Q, S = big
    tau = tau_for_hits(S, 100)
    ref = _answer(g, Q[:300], tau)
    ref70 = _answer(g, Q[:70], tau)
    try:
        g.set_image_dtype(0)                          # bf16 image: another margin, the same answer
        _same(_answer(g, Q[:300], tau), ref)
        _same(_answer(g, Q[:70], tau), ref70)
        g.set_image_dtype(1)
        g.set_option("force_exact", 1)                # f32 scorer
        _same(_answer(g, Q[:300], tau), ref)
        g.set_option("force_exact", 0)
        g.set_option("small_batch_kernel", 0)         # 70 queries through the tile kernel
        _same(_answer(g, Q[:70], tau), ref70)
    finally:
        g.set_image_dtype(1)
        g.set_option("force_exact", 0)
        g.set_option("small_batch_kernel", 1)
    check_range(*ref, S[:300], tau, BAND)


def test_norm_none_heavy_tails_and_fp16_overflow():
    from isehr_amd import _lib
    n = 30_000
    rng = np.random.default_rng(401)
    X = _gauss(402, n) * np.exp(rng.standard_normal((n, 1)) * 1.5).astype(np.float32)
    g = _lib.Gallery.from_host(X, norm_mode=_lib.NORM_NONE)
    try:
        Q = _gauss(403, 130) * 0.05
        Q[5] *= 2.0e6                                 # elements ~1e5: its fp16 image overflows (FLAG_RANGE)
        S, _, _ = host_f64_scores_and_topk(g, Q, 1, normalize_queries=False)
        for tau in (tau_for_hits(S, 50), tau_for_hits(S, 1000)):
            ans = _answer(g, Q, tau)
            check_range(*ans, S, tau, EXACT)
            g.set_option("force_exact", 1)
            try:
                _same(_answer(g, Q, tau), ans)
            finally:
                g.set_option("force_exact", 0)
        tau = float(np.sort(S[5])[-40])
        lims, idx, sc = _answer(g, Q[5:6], tau)
        check_range(lims, idx, sc, S[5:6], tau, EXACT)
        assert lims[-1] >= 40
    finally:
        g.close()


def test_global_ids_offset_and_append():
    from isehr_amd import _lib
    n = 20_000
    X = _gauss(501, n)
    Q = _gauss(502, 40)
    g = _lib.Gallery.from_host(X, norm_mode=_lib.NORM_NONE)
    go = _lib.Gallery.from_host(X, norm_mode=_lib.NORM_NONE, row_offset=1_000_000)
    ga = _lib.Gallery.empty(n, D, norm_mode=_lib.NORM_NONE, row_offset=500_000)
    try:
        S, _, _ = host_f64_scores_and_topk(g, Q, 1, normalize_queries=False)
        tau = tau_for_hits(S, 200)
        base = _answer(g, Q, tau)
        check_range(*base, S, tau, EXACT)
        lo, io, so = _answer(go, Q, tau)
        assert (lo == base[0]).all() and (io == base[1] + 1_000_000).all()
        ga.append(X[:7000])
        part = _answer(ga, Q, tau)                      # the rows appended so far, global ids
        check_range(*part, S[:, :7000], tau, EXACT, row_offset=500_000)
        ga.append(X[7000:])
        la, ia, sa = _answer(ga, Q, tau)
        assert (la == base[0]).all() and (ia == base[1] + 500_000).all()
        assert (sa.view(np.uint32) == base[2].view(np.uint32)).all()
    finally:
        g.close()
        go.close()
        ga.close()


def test_capacity_protocol(big):
    from isehr_amd import _lib
    g, Q, S = big
    tau = tau_for_hits(S, 100)
    q = np.ascontiguousarray(Q[:200])
    full = _answer(g, q, tau)
    total = int(full[0][-1])
    assert total > 10
    lims = np.full(201, -7, np.int64)
    idx = np.full(total, -3, np.int64)
    sc = np.full(total, 5.0, np.float32)
    P = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    lib = _lib.load()
    rc = lib.mi_range_search(g._h, P(q), 200, _lib.MI_F32, D, 1, tau, total - 1, P(lims), P(idx), P(sc), None)
    assert rc == _lib.MI_ERR_CAPACITY
    assert (lims == full[0]).all()
    assert (idx == -3).all() and (sc == 5.0).all()
    rc = lib.mi_range_search(g._h, P(q), 200, _lib.MI_F32, D, 1, tau, int(lims[-1]), P(lims), P(idx), P(sc), None)
    assert rc == 0
    _same((lims, idx, sc), full)
    # more than one batch: the same protocol
    q2 = np.ascontiguousarray(Q[np.arange(1100) % 1024])
    f2 = _answer(g, q2, tau)
    l2 = np.zeros(1101, np.int64)
    i2 = np.full(int(f2[0][-1]), -3, np.int64)
    rc = lib.mi_range_search(g._h, P(q2), 1100, _lib.MI_F32, D, 1, tau, int(f2[0][-1]) - 1, P(l2), P(i2), None, None)
    assert rc == _lib.MI_ERR_CAPACITY and (l2 == f2[0]).all() and (i2 == -3).all()
    lr, ir, sr, _ = g.range_search(q2, tau, max_results=5)
    _same((lr, ir, sr), f2)


def test_no_interference_with_search(big):
    import torch
    g, Q, S = big
    tau = tau_for_hits(S, 100)
    ref = g.search(Q[:300], 100)[:2]
    ref_small = g.search(Q[:50], 100)[:2]
    for _ in range(2):
        _answer(g, Q[:257], tau)
        got = g.search(Q[:300], 100)[:2]
        assert (got[0] == ref[0]).all() and (got[1].view(np.uint32) == ref[1].view(np.uint32)).all()
        _answer(g, Q[:1], tau)
        got = g.search(Q[:50], 100)[:2]
        assert (got[0] == ref_small[0]).all() and (got[1].view(np.uint32) == ref_small[1].view(np.uint32)).all()
    # a deferred tail (async_tail 3) pending from search_device when the range search starts
    k, nq = 100, 512
    q = torch.from_numpy(Q[:nq]).cuda()
    want = g.search(Q[:nq], k)[0]
    rng_ref = _answer(g, Q[:129], tau)
    ix = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    g.set_option("async_tail", 3)
    try:
        torch.cuda.synchronize()
        g.search_device(q.data_ptr(), nq, k, ix.data_ptr())       # its tail is deferred to the next call
        mid = _answer(g, Q[:129], tau)
        g.join()
        torch.cuda.synchronize()
    finally:
        g.set_option("async_tail", 0)
    assert (ix.cpu().numpy() == want).all()
    _same(mid, rng_ref)
    got = g.search(Q[:300], 100)[:2]
    assert (got[0] == ref[0]).all()


def test_knn_wrapper(big):
    from isehr_amd.knn import KNN
    X = _gauss(601, 5000)
    Q = _gauss(602, 8)
    knn = KNN(X)
    try:
        S = Q.astype(np.float64) @ X.astype(np.float64).T
        tau = tau_for_hits(S, 30)
        lims, Dv, Iv = knn.range_search(Q, tau)
        check_range(lims, Iv, Dv, S, tau, EXACT)
        assert Dv.dtype == np.float32 and Iv.dtype == np.int64
    finally:
        knn.close()


def test_full_size():
    import torch
    from isehr_amd import _lib
    N = 1005994
    s = torch.cuda.current_stream().cuda_stream
    raw = torch.empty((N, D), dtype=torch.float32, device="cuda")
    _lib.synth_fill_device(raw.data_ptr(), 4321, 0, N, D, s)
    torch.cuda.synchronize()
    g = _lib.Gallery.from_device_ptr(raw.data_ptr(), N, D)
    del raw
    try:
        from isehr_amd.synth import synth_rows
        Q = synth_rows(4322, 0, 64, D)
        S, _, _ = host_f64_scores_and_topk(g, Q, 1)
        tau = tau_for_hits(S, 100)
        lims, idx, sc, _ = g.range_search(Q, tau)
        check_range(lims, idx, sc, S, tau, BAND)
        assert 20 * 64 < lims[-1] < 500 * 64
    finally:
        g.close()


def test_near_duplicate_pairs():
    from isehr_amd import _lib
    from isehr_amd.dedup import near_duplicate_pairs
    n = 50_000
    X = _gauss(701, n)
    rng = np.random.default_rng(702)
    slots = rng.choice(n, 600, replace=False)
    for gi in range(100):                                   # 100 groups of 6: a source row and 5 (jittered) copies
        src, dst = slots[6 * gi], slots[6 * gi + 1:6 * gi + 6]
        X[dst] = X[src] + (1e-3 * (gi % 3)) * rng.standard_normal((5, D), dtype=np.float32)
    g = _lib.Gallery.from_host(X, norm_mode=_lib.NORM_NONE)
    try:
        tau = 0.9 * float(np.min(np.einsum("ij,ij->i", X[slots].astype(np.float64), X[slots].astype(np.float64))))
        i, j, s = near_duplicate_pairs(g, tau, batch=4096)
        R = g.get_rows(0, n).astype(np.float64)
        want = set()
        cand = np.unique(slots)
        sub = R[cand] @ R.T                                  # only planted rows can have partners above tau here
        for a, row in zip(cand, sub):
            for b in np.flatnonzero(row >= tau):
                if b > a:
                    want.add((int(a), int(b)))
        got = list(zip(i.tolist(), j.tolist()))
        assert len(got) == len(set(got))
        assert set(got) == want
        assert (i < j).all()
        assert np.abs(s - np.array([R[a] @ R[b] for a, b in got])).max() <= 3e-7 * max(1.0, tau)
    finally:
        g.close()
