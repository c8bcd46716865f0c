"""GPU: exact squared-L2 top-K (mi_gallery_create_l2, mi_knn_search_l2, mi_knn_search_l2_device, mi_knn_dense64_search_l2,
Gallery.search_l2, KNN(..., 'euclidean')).

Truth is numpy float64 computed here from the source rows: sum_j (q_j - x_j)^2 in the direct form on the f32 values promoted to
float64, ordered by (distance, id).  For more than a handful of queries the direct form of every row would take the host
minutes, so `l2_truth` takes it in two steps that lose nothing: (i) the float64 expansion ||q||^2 - 2 q.x + ||x||^2 of every
row (one GEMM), whose distance to the direct form is below E = 4 (D + 4) 2^-53 (||q||^2 + max ||x||^2) (standard summation
analysis of the GEMM and the three-term sum, with a factor 4 to spare); (ii) the direct form of the k + 64 rows of smallest
expansion.  A row outside them has expansion >= e, the largest expansion among them, hence direct distance >= e - E; the helper
ASSERTS that the k-th smallest direct distance lies below e - E, so the direct-form top-k of the candidates is the direct-form
top-k of all rows.

Agreement band (the selection ranks by the expansion in float64): B = (D + 4) 2^-53 (||q||^2 + ||x||^2).  `l2_truth` asserts
that consecutive true distances among the first k + 1 are either exactly equal (planted duplicate rows: ordered by id) or more
than B apart, so every id comparison below is exact equality for every query.  Returned dist64 must be within 2 D 2^-53
relative of the truth (summation order), and dist must be float32(dist64) bit for bit."""
import ctypes as C
import os
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D = 2048
U = 2.0 ** -53


def _gauss(seed, n, d=D):
    return np.random.default_rng(seed).standard_normal((n, d), dtype=np.float32)


def l2_truth(X32, Q32, k, mask=None, block=128):
    """-> (ids int64 [Q, k], dist float64 [Q, k]) by (distance asc, id asc), -1 / +inf padded; see the module docstring."""
    X = np.asarray(X32, np.float32).astype(np.float64)
    Q = np.asarray(Q32, np.float32).astype(np.float64)
    n, d = X.shape
    gn = np.einsum("ij,ij->i", X, X)
    allowed = np.arange(n) if mask is None else np.flatnonzero(mask)
    ke = min(k, len(allowed))
    ids = np.full((len(Q), k), -1, np.int64)
    dist = np.full((len(Q), k), np.inf)
    if ke == 0:
        return ids, dist
    kc = min(ke + 64, len(allowed))
    Xa, gna = X[allowed], gn[allowed]
    gmax = float(gna.max())
    for q0 in range(0, len(Q), block):
        Qb = Q[q0:q0 + block]
        qn = np.einsum("ij,ij->i", Qb, Qb)
        E = qn[:, None] - 2.0 * (Qb @ Xa.T) + gna[None, :]
        cand = np.argpartition(E, kc - 1, axis=1)[:, :kc] if kc < len(allowed) else np.tile(np.arange(len(allowed)), (len(Qb), 1))
        for i in range(len(Qb)):
            c = np.sort(allowed[cand[i]])
            diff = Qb[i][None, :] - X[c]
            dd = (diff ** 2).sum(1)
            order = np.lexsort((c, dd))
            top, td = c[order], dd[order]
            if kc < len(allowed):
                e = E[i, cand[i]].max()
                slack = 4.0 * (d + 4) * U * (qn[i] + gmax)
                assert td[ke - 1] < e - slack, "candidate set of the host truth too small: raise the 64"
            band = (d + 4) * U * (qn[i] + gn[top[:ke + 1]].max())
            gaps = np.diff(td[:ke + 1])
            assert ((gaps == 0) | (gaps > band)).all(), "two true distances inside the agreement band: change the seed"
            ids[q0 + i, :ke], dist[q0 + i, :ke] = top[:ke], td[:ke]
    return ids, dist


def check_answer(got, truth, d=D, row_offset=0):
    idx, dist, dist64 = got[0], got[1], got[2]
    tid, td = truth
    want_ids = np.where(tid >= 0, tid + row_offset, -1)
    assert (idx == want_ids).all(), "ids differ from the float64 truth at %d places" % int((idx != want_ids).sum())
    fin = np.isfinite(td)
    assert np.isposinf(dist64[~fin]).all() and np.isposinf(dist[~fin]).all()
    err = np.abs(dist64[fin] - td[fin])
    assert (err <= 2.0 * d * U * td[fin]).all(), err.max()
    assert (dist.view(np.uint32) == dist64.astype(np.float32).view(np.uint32)).all()


def dev_search(g, Q32, k):
    """the device entry point on torch tensors -> (ids, dist, dist64) host arrays; the sticky flags must be clear"""
    import torch
    dev = torch.device("cuda", 0)
    q = torch.from_numpy(np.ascontiguousarray(Q32, dtype=np.float32)).to(dev)
    nq = q.shape[0]
    idx = torch.empty((nq, k), dtype=torch.int64, device=dev)
    ds = torch.empty((nq, k), dtype=torch.float32, device=dev)
    d64 = torch.empty((nq, k), dtype=torch.float64, device=dev)
    g.search_l2_device(q.data_ptr(), nq, k, idx.data_ptr(), ds.data_ptr(), d64.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    flags = g.flags()
    return (idx.cpu().numpy(), ds.cpu().numpy(), d64.cpu().numpy()), flags


def both(g, Q32, k, truth, d=D, row_offset=0, unflagged=False):
    """the case through the host and through the device entry point.  unflagged: the device call must raise no sticky flag
    (cases at unit scale, where the record of scripts/l2_search_timing.py shows no flagged batch), so that its ids and
    distances are compared for certain; elsewhere a raised flag means 'answer again', which the host call has done."""
    host = g.search_l2(Q32, k)
    check_answer(host, truth, d, row_offset)
    got, flags = dev_search(g, Q32, k)
    if unflagged:
        assert flags == 0, flags
    if flags == 0:
        check_answer(got, truth, d, row_offset)
    return host, flags


# ---------------------------------------------------------------------------------------------------------------- varied norms
N1 = 200_000


@pytest.fixture(scope="module")
def varied():
    from isehr_amd import _lib
    rng = np.random.default_rng(11)
    X = _gauss(901, N1)
    X *= rng.uniform(0.02, 0.06, N1).astype(np.float32)[:, None]          # norms 0.9 .. 2.7
    Q = _gauss(902, 1024)
    Q *= rng.uniform(0.02, 0.06, 1024).astype(np.float32)[:, None]
    g = _lib.Gallery.l2_from_host(X)
    truth = l2_truth(X, Q, 100)
    S = Q.astype(np.float64) @ X.astype(np.float64).T               # the float64 inner-product top-K of the same data
    ip = np.argpartition(-S, 99, axis=1)[:, :100]
    del S
    yield g, X, Q, truth, ip
    g.close()


@pytest.mark.parametrize("nq", [1, 70, 1024])
def test_varied_norms(varied, nq):
    g, X, Q, (tid, td), ip = varied
    assert g.get_option("metric") == 1 and g.d == D and g.n == N1
    # the inner-product top-K of the same data is another set for EVERY query: this cannot pass on the IP path
    for i in range(nq):
        assert set(ip[i]) != set(tid[i]), i
    g.status(reset=True)
    both(g, Q[:nq], 100, (tid[:nq], td[:nq]))
    st = g.status()
    print("varied norms nq=%d: overflow_batches=%d survivors/q=%.0f candidates/q=%.0f image_f16=%d" % (
        nq, st["overflow_batches"], st["survivors"] / max(1, st["queries"]), st["candidates"] / max(1, st["queries"]),
        g.get_option("image_dtype")))


def test_checker_equals_host_truth(varied):
    g, X, Q, (tid, td), _ = varied
    idx, dist, dist64, _ = g.dense64_search_l2(Q[:96], 100)
    check_answer((idx, dist, dist64), (tid[:96], td[:96]))


# ------------------------------------------------------------------------------------------------------------------ unit rows
def test_unit_rows_agree_with_the_inner_product_search():
    from isehr_amd import _lib
    n = 50_000
    X = _gauss(911, n)
    X /= np.linalg.norm(X.astype(np.float64), axis=1)[:, None].astype(np.float32)
    Q = _gauss(912, 70)
    Q /= np.linalg.norm(Q.astype(np.float64), axis=1)[:, None].astype(np.float32)
    truth = l2_truth(X, Q, 100)
    g = _lib.Gallery.l2_from_host(X)
    gi = _lib.Gallery.from_host(X, norm_mode=_lib.NORM_NONE)
    try:
        (idx, dist, dist64, _, _), _ = both(g, Q, 100, truth, unflagged=True)
        ip_idx, _, _ = gi.search(Q, 100)
        _, _, ip64, _ = gi.dense64_search(Q, 100)
        # rows are unit length only to f32 rounding, so the two orders may differ among rows whose distances are within
        # | ||x||^2 - 1 | ~ 1e-7 of each other: as sets they agree up to those, and 2 - 2 s reproduces the distance that far
        for i in range(len(Q)):
            kth = truth[1][i, -1]
            for r in set(ip_idx[i]) ^ set(idx[i]):
                dr = ((Q[i].astype(np.float64) - X[r].astype(np.float64)) ** 2).sum()
                assert abs(dr - kth) <= 1e-6, (i, r)
        assert np.abs(np.sort(2.0 - 2.0 * ip64, axis=1) - dist64).max() <= 1e-6
    finally:
        g.close()
        gi.close()


# -------------------------------------------------------------------------------------------------- self queries and duplicates
def test_self_queries_and_duplicates():
    from isehr_amd import _lib
    n = 30_000
    rng = np.random.default_rng(21)
    X = _gauss(921, n) * rng.uniform(0.02, 0.06, n).astype(np.float32)[:, None]
    src = np.array([5, 777, 12_345, 29_999])
    for j, r in enumerate(src):                                # three more copies of each, at higher AND lower ids
        for c in (r // 2 + 1 + j, (r + 4000 + j) % n, (r + 9000 + j) % n):
            X[c] = X[r]
    Q = np.concatenate([X[src], X[[100, 200, 300]]])
    truth = l2_truth(X, Q, 100)
    g = _lib.Gallery.l2_from_host(X)
    try:
        (idx, dist, dist64, _, _), _ = both(g, Q, 100, truth)
        for j, r in enumerate(src):
            copies = np.sort(np.flatnonzero((X == X[r]).all(1)))
            assert len(copies) == 4
            assert (idx[j, :4] == copies).all()                 # the lowest id first, duplicates by id
            assert (dist64[j, :4] == 0.0).all() and (dist[j, :4] == 0.0).all()      # exactly zero, not rounding noise
        assert (dist64[4:, 0] == 0.0).all() and (idx[4:, 0] == [100, 200, 300]).all()
    finally:
        g.close()


# ------------------------------------------------------------------------------------------------ large and heavy-tailed norms
@pytest.mark.parametrize("kind", ["times30", "lognormal"])
def test_large_and_heavy_tailed_norms(kind):
    from isehr_amd import _lib
    n = 100_000
    rng = np.random.default_rng(31)
    X = _gauss(931, n)
    Q = _gauss(932, 70)
    if kind == "times30":
        X *= (30.0 * rng.uniform(0.02, 0.06, n)).astype(np.float32)[:, None]
        Q *= (30.0 * rng.uniform(0.02, 0.06, 70)).astype(np.float32)[:, None]
    else:
        X *= (0.04 * rng.lognormal(0.0, 1.0, n)).astype(np.float32)[:, None]
        Q *= (0.04 * rng.lognormal(0.0, 1.0, 70)).astype(np.float32)[:, None]
    truth = l2_truth(X, Q, 100)
    g = _lib.Gallery.l2_from_host(X)
    try:
        if kind == "times30":
            assert g.get_option("image_dtype") == 0            # 1/2 ||x||^2 up to ~3300: the bf16 image
        g.status(reset=True)
        _, flags = both(g, Q, 100, truth)
        st = g.status()
        print("%s: image_f16=%d device flags=%d overflow_batches=%d survivors=%d candidates=%d queries=%d" % (
            kind, g.get_option("image_dtype"), flags, st["overflow_batches"], st["survivors"], st["candidates"], st["queries"]))
    finally:
        g.close()


def test_bias_beyond_fp16_range_takes_the_bf16_image():
    """Every row at norm 400 .. 1100: 1/2 ||g||^2 = 80 000 .. 605 000 is beyond fp16's 65 504 while every element (~10 .. 25) fits
    it easily.  The gallery must take the bf16 image, and the ids must be the float64 truth."""
    from isehr_amd import _lib
    n = 40_000
    rng = np.random.default_rng(33)
    X = _gauss(933, n)
    X *= (rng.uniform(400.0, 1100.0, n) / np.linalg.norm(X.astype(np.float64), axis=1)).astype(np.float32)[:, None]
    Q = _gauss(934, 70)
    Q *= (rng.uniform(400.0, 1100.0, 70) / np.linalg.norm(Q.astype(np.float64), axis=1)).astype(np.float32)[:, None]
    assert np.linalg.norm(X.astype(np.float64), axis=1).min() >= 399.0
    truth = l2_truth(X, Q, 100)
    g = _lib.Gallery.l2_from_host(X)
    try:
        assert g.get_option("image_dtype") == 0
        both(g, Q, 100, truth)
        check_answer(g.dense64_search_l2(Q, 100), truth)
    finally:
        g.close()
    # a gallery whose rows straddle the limit (norms 300 .. 420: some biases fit fp16, some do not)
    X2 = _gauss(935, 5000)
    X2 *= (rng.uniform(300.0, 420.0, 5000) / np.linalg.norm(X2.astype(np.float64), axis=1)).astype(np.float32)[:, None]
    g = _lib.Gallery.l2_from_host(X2)
    try:
        assert g.get_option("image_dtype") == 0
        check_answer(g.search_l2(Q[:20], 100), l2_truth(X2, Q[:20], 100))
    finally:
        g.close()


def _split_bias(X32, f16):
    """numpy restatement of l2_bias_kernel (tests/test_l2_search_cpu.py): the three hidden columns of every row"""
    g = X32.astype(np.float64)
    b = -0.5 * (g * g).sum(1)
    b32 = b.astype(np.float32)
    if f16:
        with np.errstate(over="ignore"):
            c1 = b32.astype(np.float16).astype(np.float32)
        c1 = np.where(np.isfinite(c1), c1, np.float32(-65504.0)).astype(np.float32)   # beyond fp16: its largest finite value
    else:
        u = b32.view(np.uint32).astype(np.uint64)
        c1 = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32)
    c2 = (b - c1.astype(np.float64)).astype(np.float32)
    c3 = (b - c1.astype(np.float64) - c2.astype(np.float64)).astype(np.float32)
    return np.stack([c1, c2, c3], 1)


def test_equals_a_gallery_ingested_with_the_columns():
    """An L2 gallery against a MI_NORM_NONE gallery ingested from the array [g, c1, c2, c3] (the split restated in numpy), searched
    with [q, 1, 1, 1].  This is NOT the section-by-section equality the two galleries should have: the image and RowStat
    sections are pinned element by element in tests/test_gpu_l2_gallery_reference.py (the saved file, read back on the host); a
    few misplaced elements or a norm a few per cent off would pass here.  What the test does pin is what depends on the sections:
    the float64 inner-product scores of the augmented gallery reproduce the L2 distances (f32 section),
    both return the same rows, and the filter keeps and passes on to the exact re-score the same number of rows within a few
    per cent (image and RowStat sections: a wrong swizzle or a misplaced hidden column changes every approximate score, a wrong
    norm the margin; the norms are summed in another order than the ingest's, so the margins may differ in the last place)."""
    from isehr_amd import _lib
    n = 30_000
    X = _gauss(936, n) * np.random.default_rng(36).uniform(0.01, 0.03, n).astype(np.float32)[:, None]     # norms 0.45 .. 1.36: fp16
    Q = _gauss(937, 300) * np.float32(0.02)
    g = _lib.Gallery.l2_from_host(X)
    assert g.get_option("image_dtype") == 1
    A = np.concatenate([X, _split_bias(X, True)], 1)
    QA = np.concatenate([Q, np.ones((len(Q), 3), np.float32)], 1)
    gi = _lib.Gallery.from_host(A, norm_mode=_lib.NORM_NONE)
    try:
        assert gi.get_option("image_dtype") == 1
        for h in (g, gi):
            h.set_option("boot_ksplit", 0)                     # fixed summation order of the sample scores
            h.set_option("ladder", 0)                          # no threshold that depends on the order the tiles finish in
        for nq in (300, 16):
            g.status(reset=True)
            idx, _, dist64, _, _ = g.search_l2(Q[:nq], 100)
            st = g.status()
            gi.status(reset=True)
            _, _, s64, _ = gi.dense64_search(QA[:nq], 100)
            ip_idx, _, _ = gi.search(QA[:nq], 100)
            sti = gi.status()
            assert st["overflow_batches"] == 0 and sti["overflow_batches"] == 0
            assert (np.sort(idx, 1) == np.sort(ip_idx, 1)).all()
            qn = (Q[:nq].astype(np.float64) ** 2).sum(1)[:, None]
            assert np.abs((qn - 2.0 * s64) - dist64).max() <= 1e-12
            assert abs(st["candidates"] - sti["candidates"]) <= 0.02 * sti["candidates"] + 2
            assert abs(st["survivors"] - sti["survivors"]) <= 0.05 * sti["survivors"] + 2
    finally:
        g.close()
        gi.close()


def test_whitened_append():
    """mi_gallery_append_whitened_device on an L2 gallery (rows stored un-normalised: MI_NORM_NONE): P (x - m) of the appended
    rows, rounded to f32, equal to a one-shot gallery of those rows in get_rows, ids and dist64."""
    import torch
    from isehr_amd import _lib
    n, d_in, d = 1500, 160, 128
    rng = np.random.default_rng(38)
    Xin = rng.standard_normal((n, d_in)).astype(np.float32)
    P = (rng.standard_normal((d, d_in)) * 0.1).astype(np.float64)
    m = rng.standard_normal(d_in).astype(np.float64) * 0.1
    Y = ((Xin.astype(np.float64) - m[None, :]) @ P.T).astype(np.float32)
    Qy = Y[[3, 700, 1499]] + np.float32(0.01)
    dev = torch.device("cuda", 0)
    xt, pt, mt = torch.from_numpy(Xin).to(dev), torch.from_numpy(P).to(dev), torch.from_numpy(m).to(dev)
    torch.cuda.synchronize()
    app = _lib.Gallery.l2_from_host(None, d=d, capacity=n)
    try:
        s = torch.cuda.current_stream().cuda_stream
        app.append_whitened_device(xt.data_ptr(), 1000, d_in, mt.data_ptr(), pt.data_ptr(), stream=s)
        app.append_whitened_device(xt[1000:].data_ptr(), 500, d_in, mt.data_ptr(), pt.data_ptr(), stream=s)
        stored = app.get_rows(0, n)
        assert stored.shape == (n, d) and np.abs(stored.astype(np.float64) - Y).max() <= 1e-5
        one = _lib.Gallery.l2_from_host(stored)
        try:
            a, b = app.search_l2(Qy, 50), one.search_l2(Qy, 50)
            check_answer(a, l2_truth(stored, Qy, 50), d)
            assert (a[0] == b[0]).all() and (a[2].view(np.uint64) == b[2].view(np.uint64)).all()
        finally:
            one.close()
    finally:
        app.close()


# --------------------------------------------------------------------------------------------------------------------- shapes
@pytest.mark.parametrize("d", [64, 100, 2048])
def test_shapes(d):
    from isehr_amd import _lib
    n = 5000
    rng = np.random.default_rng(41 + d)
    X = _gauss(941 + d, n, d) * rng.uniform(0.5, 1.5, n).astype(np.float32)[:, None]
    Q = _gauss(942 + d, 33, d) * rng.uniform(0.5, 1.5, 33).astype(np.float32)[:, None]
    g = _lib.Gallery.l2_from_host(X, row_offset=1000)
    g64 = _lib.Gallery.l2_from_host(np.asfortranarray(X.astype(np.float64)))        # float64, [D, N]-strided source
    try:
        assert g.d == d and g64.d == d
        assert (g.get_rows(0, n).view(np.uint32) == X.view(np.uint32)).all()        # the hidden columns never leave
        assert (g64.get_rows(0, n).view(np.uint32) == X.view(np.uint32)).all()
        for k in (1, 100, 2048):
            truth = l2_truth(X, Q, k)
            both(g, Q, k, truth, d, row_offset=1000)
            check_answer(g64.search_l2(np.asfortranarray(Q.astype(np.float64)), k), truth, d)   # f64, strided queries
            check_answer(g.dense64_search_l2(Q, k), truth, d, row_offset=1000)
    finally:
        g.close()
        g64.close()


def test_fewer_rows_than_k_and_more_than_one_batch():
    from isehr_amd import _lib
    X = _gauss(951, 37, 100)
    Q = _gauss(952, 1500, 100)                                                       # nq > 1024 through the host call
    truth = l2_truth(X, Q, 50)
    assert (truth[0][:, 37:] == -1).all()
    g = _lib.Gallery.l2_from_host(X)
    try:
        both(g, Q, 50, truth, 100)
        check_answer(g.dense64_search_l2(Q[:20], 50), (truth[0][:20], truth[1][:20]), 100)
    finally:
        g.close()
    n = 20_000
    X = _gauss(953, n) * np.random.default_rng(5).uniform(0.02, 0.06, n).astype(np.float32)[:, None]
    Q = _gauss(954, 1100)
    Q *= np.float32(0.04)
    g = _lib.Gallery.l2_from_host(X)
    try:
        check_answer(g.search_l2(Q, 100), l2_truth(X, Q, 100))
    finally:
        g.close()


# --------------------------------------------------------------------------------------------------------------------- append
def test_append_equals_one_shot():
    import torch
    from isehr_amd import _lib
    n = 3000
    X = _gauss(961, n) * np.random.default_rng(6).uniform(0.02, 0.06, n).astype(np.float32)[:, None]
    Q = np.concatenate([_gauss(962, 40) * np.float32(0.04), X[[0, 999, 2999]]])
    one = _lib.Gallery.l2_from_host(X)
    app = _lib.Gallery.l2_from_host(X[:200], capacity=n)
    emp = _lib.Gallery.l2_from_host(None, d=D, capacity=n)
    try:
        # 200 | strided host append crossing the 256-row tile | device append | the rest from a [D, N] block
        app.append(np.asfortranarray(X[200:700]))
        t = torch.from_numpy(X[700:1500]).to("cuda:0")
        torch.cuda.synchronize()
        app.append_device(t.data_ptr(), 800, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        app.append(np.ascontiguousarray(X[1500:].T).T)
        emp.append(X[:1000])
        emp.append(X[1000:])
        ref = one.search_l2(Q, 100)
        check_answer(ref, l2_truth(X, Q, 100))
        for g in (app, emp):
            assert g.n == n and g.d == D
            assert (g.get_rows(0, n).view(np.uint32) == one.get_rows(0, n).view(np.uint32)).all()
            got = g.search_l2(Q, 100)
            assert (got[0] == ref[0]).all()
            assert (got[2].view(np.uint64) == ref[2].view(np.uint64)).all()
            assert (got[1].view(np.uint32) == ref[1].view(np.uint32)).all()
    finally:
        for g in (one, app, emp):
            g.close()


# ------------------------------------------------------------------------------------------------------------------- filtered
def test_filtered_paths():
    from isehr_amd import _lib
    n = 60_000
    X = _gauss(971, n) * np.random.default_rng(7).uniform(0.02, 0.06, n).astype(np.float32)[:, None]
    Q = _gauss(972, 70) * np.float32(0.04)
    g = _lib.Gallery.l2_from_host(X)
    try:
        for sel in (0.3, 0.01):
            mask = np.random.default_rng(8).random(n) < sel
            truth = l2_truth(X, Q, 100, mask)
            for path in (1, 2):
                g.set_option("filter_path", path)
                got = g.search_l2(Q, 100, allow=mask)
                assert got[3]["path"] == path and got[3]["allowed"] == int(mask.sum())
                check_answer(got, truth)
        g.set_option("filter_path", 0)
        five = np.zeros(n, bool)
        five[[3, 4000, 4001, 50_000, 59_999]] = True
        check_answer(g.search_l2(Q, 100, allow=five), l2_truth(X, Q, 100, five))
        none = g.search_l2(Q, 100, allow=np.zeros(n, bool))
        assert (none[0] == -1).all() and np.isposinf(none[2]).all()
        ref = g.search_l2(Q, 100)
        for path in (0, 1, 2):
            g.set_option("filter_path", path)
            got = g.search_l2(Q, 100, allow=np.ones(n, bool))
            assert (got[0] == ref[0]).all() and (got[2].view(np.uint64) == ref[2].view(np.uint64)).all()
            assert (got[1].view(np.uint32) == ref[1].view(np.uint32)).all()
    finally:
        g.close()


# ------------------------------------------------------------------------------------------------------------------ full size
def test_full_size_main_path_equals_the_checker():
    """1 005 994 x 2048 synthetic rows scaled per row, K = 100, 1024 queries: the main path equals the dense checker id for id,
    and 8 of the queries are scored on the host in float64 over ALL rows (direct form, 64 k-row chunks of get_rows)."""
    import torch
    from isehr_amd import _lib
    from isehr_amd.synth import synth_rows
    N, K = 1_005_994, 100
    dev = torch.device("cuda", 0)
    raw = torch.empty((N, D), dtype=torch.float32, device=dev)
    _lib.synth_fill_device(raw.data_ptr(), 1234, 0, N, D, torch.cuda.current_stream().cuda_stream)
    scale = np.random.default_rng(77).uniform(0.5, 1.5, N).astype(np.float32) * np.float32(1.0 / 52.0)      # norms ~0.5 .. 1.5
    raw *= torch.from_numpy(scale).to(dev)[:, None]
    Q = synth_rows(4321, 0, 1024, D) * (np.random.default_rng(78).uniform(0.5, 1.5, 1024).astype(np.float32) / np.float32(52.0))[:, None]
    torch.cuda.synchronize()
    g = _lib.Gallery.l2_from_device_ptr(raw.data_ptr(), N, D)
    del raw
    torch.cuda.empty_cache()
    try:
        g.status(reset=True)
        idx, dist, dist64, _, _ = g.search_l2(Q, K)
        st = g.status()
        print("full size: overflow_batches=%d survivors/q=%.0f candidates/q=%.0f image_f16=%d" % (
            st["overflow_batches"], st["survivors"] / 1024, st["candidates"] / 1024, g.get_option("image_dtype")))
        cidx, cdist, cdist64, _ = g.dense64_search_l2(Q, K)
        assert (idx == cidx).all()
        assert np.abs(dist64 - cdist64).max() <= 2.0 * D * U * cdist64.max()
        (didx, _, dd64), flags = dev_search(g, Q, K)
        assert flags == 0                       # unit scale: nothing flagged, the device answer is compared for certain
        assert (didx == idx).all() and (dd64.view(np.uint64) == dist64.view(np.uint64)).all()
        pick = np.array([0, 1, 2, 5, 77, 300, 640, 1023])
        q8 = Q[pick].astype(np.float64)
        all_d = np.empty((8, N))
        for r0 in range(0, N, 65536):
            rows = g.get_rows(r0, min(65536, N - r0)).astype(np.float64)
            for i in range(8):
                all_d[i, r0:r0 + len(rows)] = ((q8[i][None, :] - rows) ** 2).sum(1)
        for i, qi in enumerate(pick):
            order = np.lexsort((np.arange(N), all_d[i]))[:K + 1]
            band = (D + 4) * U * ((q8[i] ** 2).sum() + 1.5 ** 2 * 1.1)
            assert (np.diff(all_d[i][order]) > band).all(), "two true distances inside the agreement band: change the seed"
            assert (idx[qi] == order[:K]).all(), qi
            assert (np.abs(dist64[qi] - all_d[i][order[:K]]) <= 2.0 * D * U * all_d[i][order[:K]]).all()
    finally:
        g.close()


# -------------------------------------------------------------------------------------------------------------------- surface
def test_surface():
    from isehr_amd import _lib
    from isehr_amd.knn import KNN
    lib = _lib.load()
    X = _gauss(981, 4000, 128) * np.random.default_rng(9).uniform(0.5, 1.5, 4000).astype(np.float32)[:, None]
    Q = _gauss(982, 9, 128)
    knn = KNN(X, "euclidean")
    try:
        dist, ids = knn.search(Q.astype(np.float64), 10)
        assert dist.dtype == np.float32 and ids.dtype == np.int64 and dist.shape == ids.shape == (9, 10)
        tid, td = l2_truth(X, Q, 10)
        assert (ids == tid).all() and (dist == td.astype(np.float32)).all() and (np.diff(dist, axis=1) >= 0).all()
        mask = np.arange(4000) % 3 == 0
        dist, ids = knn.search(Q, 10, allow=mask)
        assert (ids == l2_truth(X, Q, 10, mask)[0]).all()
        with pytest.raises(NotImplementedError):
            knn.range_search(Q, 1.0)
        g = knn.gallery
        P = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
        idx = np.zeros((9, 10), np.int64)
        sc = np.zeros((9, 10), np.float32)
        lims = np.zeros(10, np.int64)
        bits = _lib.allow_bitmap(mask, 4000)
        refused = [
            lib.mi_knn_search(g._h, P(Q), 9, 0, 128, 1, 10, P(idx), P(sc), None),
            lib.mi_knn_search_device(g._h, P(Q), 9, 10, P(idx), None, None, None),
            lib.mi_knn_search_filtered(g._h, P(Q), 9, 0, 128, 1, 10, P(bits), 0, P(idx), P(sc), None, None),
            lib.mi_range_search(g._h, P(Q), 9, 0, 128, 1, 0.5, 10, P(lims), P(idx), P(sc), None),
            lib.mi_knn_dense_search(g._h, P(Q), 9, 0, 128, 1, 10, P(idx), P(sc), None),
            lib.mi_knn_dense64_search(g._h, P(Q), 9, 0, 128, 1, 10, P(idx), P(sc), None, None),
            lib.mi_gallery_set_image_dtype(g._h, 0),
            lib.mi_knn_phase1_device(g._h, P(Q), 9, 10, P(sc), None),
            lib.mi_online_create(g._h, None, 10, 3, 4.0, 1e-6, 8, 100, C.byref(C.c_void_p())),
            lib.mi_diffusion_set_offline(g._h, P(idx), P(sc), 10),
        ]
        assert refused == [_lib.MI_ERR_UNSUPPORTED] * len(refused), refused
        assert b"MI_METRIC_L2" in lib.mi_last_error()
        # save / load keep the metric: the loaded gallery answers bit for bit like the original
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "l2.gal")
            g.save(path)
            loaded = _lib.Gallery.load(path)
        try:
            assert loaded.get_option("metric") == 1 and (loaded.n, loaded.d) == (g.n, g.d)
            a, b = g.search_l2(Q, 10), loaded.search_l2(Q, 10)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
            assert np.array_equal(a[2].view(np.uint64), b[2].view(np.uint64)) and (a[0] == tid).all()
        finally:
            loaded.close()
        # what keeps working on the caller's d
        assert g.d == 128 and g.get_rows(0, 3).shape == (3, 128)
        assert g.scatter().shape == (128, 128)
        g.calibrate(2)
        assert g.flags() == 0 and g.status()["queries"] > 0
        with pytest.raises(RuntimeError):
            g.set_option("metric", 0)                                  # read-only
    finally:
        knn.close()
    gi = _lib.Gallery.from_host(X, norm_mode=_lib.NORM_NONE)
    try:
        assert gi.get_option("metric") == 0
        d64 = np.zeros((9, 10), np.float64)
        assert lib.mi_knn_search_l2(gi._h, P(Q), 9, 0, 128, 1, 10, None, 0, P(idx), P(sc), P(d64), None, None) == _lib.MI_ERR_INVALID
        assert lib.mi_knn_search_l2_device(gi._h, P(Q), 9, 10, P(idx), None, None, None) == _lib.MI_ERR_INVALID
        assert lib.mi_knn_dense64_search_l2(gi._h, P(Q), 9, 0, 128, 1, 10, P(idx), P(sc), P(d64), None) == _lib.MI_ERR_INVALID
    finally:
        gi.close()
