"""GPU: exact re-ranking of index shortlists on the raw rows (mi_refine, mi_refine_device, Gallery.refine, the refine= option of the
four index searches, knn.ANN(refine_k_factor=)) against the numpy float64 truth of tests/_refine_truth.py.

Ids must EQUAL the truth: the inputs are seeded so that no two distinct candidates of a query lie within twice the rounding bound
(d + 4) 2^-53 (||q||^2 + ||g||^2) of each other (asserted here on the host, and for the whole sweep in test_refine_cpu.py); val64
must lie within that bound of the truth and val must be float32(val64)."""
import numpy as np
import pytest

import _refine_truth as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from isehr_amd import _lib
    _lib.load()
    return _lib


def _gallery(lib, rows, l2, off=0, norm=None):
    if l2:
        return lib.Gallery.l2_from_host(rows, row_offset=off)
    return lib.Gallery.from_host(rows, norm_mode=lib.NORM_NONE if norm is None else norm, row_offset=off)


def _check(lib, g, rows, q, cand, k, l2, off=0, gap=True):
    d = rows.shape[1]
    if gap:
        assert T.min_gap_over_bound(rows, q, cand, l2, off) > 2.0
    ids, val, val64, _ = g.refine(q, cand, k)
    tid, tval = T.refine_truth(rows, q, cand, k, l2, off)
    bound = T.value_bound(rows, q, tid, d, off)
    real = tid >= 0
    with np.errstate(invalid="ignore"):                                    # (inf - inf at the padding)
        err = np.abs(np.where(real, val64 - tval, 0.0))
    print("refine: max |val64 - truth| / bound = %.3g" % float((err[real] / bound[real]).max() if real.any() else 0.0))
    assert np.array_equal(ids, tid)
    assert (err <= bound).all()
    assert np.array_equal(val64[~real], tval[~real])                       # padding: +inf / -inf
    assert np.array_equal(val, val64.astype(np.float32))
    return ids, val64


@pytest.mark.parametrize("case", T.sweep_cases(), ids=lambda c: "kc%d-d%d-N%d-nq%d-%s-%s-off%d" % (c[0], c[1], c[2], c[3], c[4], "l2" if c[5] else "ip", c[6]))
def test_shape_sweep(lib, case):
    kc, d, n, nq, kmode, l2, off = case
    rows, q, cand = T.case_inputs(case)
    g = _gallery(lib, rows, l2, off)
    try:
        _check(lib, g, rows, q, cand, T.k_of(kc, kmode), l2, off)
    finally:
        g.close()


@pytest.mark.parametrize("l2", [True, False])
def test_edge_cases(lib, l2):
    rng = np.random.default_rng(11)
    n, d, off = 300, 37, 5000
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((4, d)).astype(np.float32)
    g = _gallery(lib, rows, l2, off)
    try:
        base = np.stack([rng.permutation(n)[:64] for _ in range(4)]).astype(np.int64) + off
        _check(lib, g, rows, q, np.repeat(base, 2, axis=1), 64, l2, off)                     # every id twice: 64 distinct
        _check(lib, g, rows, q, np.concatenate([base, base[:, ::-1]], axis=1), 128, l2, off)  # k beyond them: padded tail
        one = np.full((4, 257), off + 17, np.int64)
        ids, val64 = _check(lib, g, rows, q, one, 257, l2, off)                               # one id kc times
        assert (ids[:, 0] == off + 17).all() and (ids[:, 1:] == -1).all()
        for pad in (np.full((4, 65), -1, np.int64), np.full((4, 65), off - 1, np.int64), np.full((4, 65), off + n, np.int64),
                    np.full((4, 65), 17, np.int64), np.full((4, 3000), np.iinfo(np.int64).min, np.int64)):
            ids, val64 = _check(lib, g, rows, q, pad, pad.shape[1] // 2 + 1, l2, off)        # all padding
            assert (ids == -1).all() and (val64 == (np.inf if l2 else -np.inf)).all()
        edge = np.array([[off - 1, off, off + n - 1, off + n, -1, 0]] * 4, np.int64)          # the shard's two ends
        ids, _ = _check(lib, g, rows, q, edge, 6, l2, off)
        assert (np.sort(ids[:, :2], axis=1) == [off, off + n - 1]).all() and (ids[:, 2:] == -1).all()
        if l2:                                                                                # a query equal to a stored row
            ids, _, val64, _ = g.refine(rows[[5, 250]], np.tile(np.arange(off, off + n), (2, 1)), 3)
            assert ids[:, 0].tolist() == [off + 5, off + 250] and (val64[:, 0] == 0.0).all() and not np.signbit(val64[:, 0]).any()
    finally:
        g.close()


def test_device_form_with_a_candidate_stride(lib):
    import torch
    rng = np.random.default_rng(12)
    n, d, nq, kc, k, stride = 700, 130, 5, 300, 40, 333
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    cand = rng.integers(-3, n + 3, size=(nq, stride)).astype(np.int64)
    for l2 in (True, False):
        g = _gallery(lib, rows, l2)
        try:
            want = g.refine(q, cand[:, :kc], k)
            tq, tc = torch.from_numpy(q).cuda(), torch.from_numpy(cand).cuda()
            idx = torch.full((nq, k), -7, dtype=torch.int64, device="cuda")
            v64 = torch.zeros((nq, k), dtype=torch.float64, device="cuda")
            s = torch.cuda.current_stream().cuda_stream
            g.refine_device(tq.data_ptr(), nq, tc.data_ptr(), kc, k, idx.data_ptr(), val64_ptr=v64.data_ptr(), stream=s, cand_stride=stride)
            assert np.array_equal(idx.cpu().numpy(), want[0]) and np.array_equal(v64.cpu().numpy(), want[2])
            g.refine_device(tq.data_ptr(), nq, tc.data_ptr(), kc, k, idx.data_ptr(), stream=s, cand_stride=stride)   # no value outputs
            assert np.array_equal(idx.cpu().numpy(), want[0])
            tid, _ = T.refine_truth(rows, q, cand[:, :kc], k, l2)
            assert np.array_equal(want[0], tid)
        finally:
            g.close()


def test_l2_bits_of_the_flat_search(lib):
    """refine over EVERY row, shuffled, gives the ids and the dist64 bits of Gallery.search_l2: both run l2_direct_wave."""
    rng = np.random.default_rng(13)
    n, d, nq = 2000, 130, 9
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    g = lib.Gallery.l2_from_host(rows, row_offset=77)
    try:
        ids, dist, dist64, _, _ = g.search_l2(q, 100)
        cand = np.stack([rng.permutation(n) for _ in range(nq)]).astype(np.int64) + 77
        rid, rval, rval64, _ = g.refine(q, cand, 100)
        assert np.array_equal(rid, ids)
        assert np.array_equal(rval64.view(np.uint64), dist64.view(np.uint64))
        assert np.array_equal(rval.view(np.uint32), dist.view(np.uint32))
    finally:
        g.close()


def test_ip_against_the_flat_search(lib):
    """The inner-product twin: the ids and the score64 BITS of mi_knn_search_device on a MI_NORM_NONE gallery.  rescore_kernel
    (select.hip) gives lane l the columns 4 l + 256 j in ascending order, x y z w within a float4, and reduces with the same
    xor-shuffle tree; its products of promoted float32 values are exact in float64, so each of its additions rounds once, exactly
    like refine's FMA, and the zero padding columns it also walks add nothing."""
    import torch
    rng = np.random.default_rng(14)
    n, d, nq, k = 2000, 130, 9, 100
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    g = lib.Gallery.from_host(rows, norm_mode=lib.NORM_NONE)
    try:
        tq = torch.from_numpy(q).cuda()
        idx = torch.empty((nq, k), dtype=torch.int64, device="cuda")
        s64 = torch.empty((nq, k), dtype=torch.float64, device="cuda")
        g.search_device(tq.data_ptr(), nq, k, idx.data_ptr(), score64_ptr=s64.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert g.flags() == 0
        cand = np.stack([rng.permutation(n) for _ in range(nq)]).astype(np.int64)
        assert T.min_gap_over_bound(rows, q, cand, False) > 2.0
        rid, _, rval64, _ = g.refine(q, cand, k)
        assert np.array_equal(rid, idx.cpu().numpy())
        assert np.array_equal(rval64.view(np.uint64), s64.cpu().numpy().view(np.uint64))
    finally:
        g.close()


def test_ip_on_a_normalised_gallery_uses_the_stored_row(lib):
    rng = np.random.default_rng(15)
    n, d = 500, 96
    rows = (rng.standard_normal((n, d)) * 3.0).astype(np.float32)
    q = rng.standard_normal((3, d)).astype(np.float32)
    g = lib.Gallery.from_host(rows, norm_mode=lib.NORM_L2, row_offset=10)
    try:
        stored = g.get_rows(0, n)
        assert np.allclose((stored.astype(np.float64) ** 2).sum(1), 1.0, atol=1e-5)
        cand = rng.integers(8, n + 12, size=(3, 200)).astype(np.int64)
        _check(lib, g, stored, q, cand, 50, False, 10)
    finally:
        g.close()


def test_refine_after_remove(lib):
    rng = np.random.default_rng(16)
    n, d, off = 400, 20, 100
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((6, d)).astype(np.float32)
    g = lib.Gallery.l2_from_host(rows, row_offset=off)
    try:
        kept = g.remove(rng.permutation(n)[:150] + off)
        left = rows[kept - off]
        assert g.n == 250 and len(kept) == 250
        cand = rng.integers(off - 2, off + n, size=(6, 128)).astype(np.int64)      # ids at or beyond off + 250 are padding now
        _check(lib, g, left, q, cand, 128, True, off)
    finally:
        g.close()


# ---- composition with the four index types: one clustered set, tie-free in float64
N, D, NQ, K, F = 5000, 64, 40, 10, 10


@pytest.fixture(scope="module")
def clustered(lib):
    rng = np.random.default_rng(21)
    centres = rng.standard_normal((16, D)) * 4.0
    x = (centres[rng.integers(0, 16, N)] + rng.standard_normal((N, D))).astype(np.float32)
    q = (centres[rng.integers(0, 16, NQ)] + rng.standard_normal((NQ, D))).astype(np.float32)
    g = lib.Gallery.l2_from_host(x)
    assert T.min_gap_over_bound(x, q, np.tile(np.arange(N), (NQ, 1)), True) > 2.0
    yield x, q, g
    g.close()


def _compose(index_search, x, q, g, lib, **kw):
    """index.search(q, K, refine=g, k_factor=F) == g.refine(q, index.search(q, K * F)[0], K), and refine=None changes nothing."""
    short = index_search(K * F, **kw)
    want = g.refine(q, short[0], K)
    got = index_search(K, refine=g, k_factor=F, **kw)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    tid, _ = T.refine_truth(x, q, short[0], K, True)
    assert np.array_equal(got[0], tid)
    plain, again = index_search(K, **kw), index_search(K, refine=None, **kw)
    assert np.array_equal(plain[0], again[0]) and np.array_equal(plain[1], again[1]) and plain[1].dtype == again[1].dtype
    return short, got, plain


def test_compose_pq(lib, clustered):
    x, q, g = clustered
    cb, _ = lib.pq_train(x, 8, 64, iters=5, seed=0)
    with lib.PQIndex.empty(cb, N) as index:
        index.add(x)
        _compose(lambda k, **kw: index.search(q, k, **kw), x, q, g, lib)
        allow = np.arange(0, N, 3)
        _compose(lambda k, **kw: index.search(q, k, allow=allow, **kw), x, q, g, lib)


def test_compose_ivfpq_and_recall(lib, clustered):
    x, q, g = clustered
    coarse, cb, _, _ = lib.IVFPQIndex.train(x, 16, 8, 256, iters=5, seed=0)
    with lib.IVFPQIndex.empty(coarse, cb, N) as index:
        index.add(x)
        short, got, plain = _compose(lambda k, **kw: index.search(q, k, nprobe=4, **kw), x, q, g, lib)
        # every true neighbour that reached the shortlist must be in the refined top-k: a miss means the kernel lost a row
        true_ids = g.search_l2(q, K)[0]
        for i in range(NQ):
            reach = set(true_ids[i]) & set(short[0][i])
            assert reach <= set(got[0][i]), i
            assert len(set(true_ids[i]) & set(got[0][i])) >= len(set(true_ids[i]) & set(plain[0][i])), i


def test_compose_hamming_and_lsh(lib, clustered):
    x, q, g = clustered
    with lib.LSHIndex.from_host(x, nbits=64) as index:
        _compose(lambda k, **kw: index.search(q, k, **kw), x, q, g, lib)
        qcodes = index.encode(q)

        def binary(k, **kw):
            if kw.get("refine") is not None:
                kw["refine_queries"] = q
            return index.gallery.search(qcodes, k, **kw)
        _compose(binary, x, q, g, lib)
        with pytest.raises(ValueError):
            index.gallery.search(qcodes, K, refine=g)                # the raw queries are missing
        with pytest.raises(ValueError):
            index.search(q, K, refine=g, k_factor=0)


def test_ann_with_refinement(lib, clustered):
    x, q, _ = clustered
    from isehr_amd.knn import ANN
    ann = ANN(x, "euclidean", M=8, nlist=16, nprobe=4, refine_k_factor=F)
    try:
        dist, ids = ann.search(q, K)
        short = ann.index.search(q, K * F, nprobe=4)[0]
        tid, tval = T.refine_truth(x, q, short, K, True)
        assert np.array_equal(ids, tid)
        assert (np.diff(dist, axis=1) >= 0).all()
        b = T.value_bound(x, q, tid, D)
        assert (np.abs(dist.astype(np.float64) - tval) <= b + (np.abs(tval) + b) * 2.0 ** -24).all()   # float32(val64)
        assert ann.remove_ids(np.arange(0, 50)) == 50 and ann.rows.n == ann.index.n == N - 50
        dist, ids = ann.search(q, K)
        short = ann.index.search(q, K * F, nprobe=4)[0]
        assert np.array_equal(ids, T.refine_truth(x[50:], q, short, K, True)[0])
    finally:
        ann.close()


def test_matchers_with_refine_rows(lib, clustered):
    x, q, g = clustered
    from isehr_amd import nnsearch
    plain, _ = nnsearch.matching_LSH_hip(K, x, q, 64)
    fine, _ = nnsearch.matching_LSH_hip(K, x, q, 64, refine_rows=x, k_factor=F)
    with lib.LSHIndex.from_host(x, R=lib.lsh_rotation(D, 64, 5)) as index:
        assert np.array_equal(plain, index.search(q, K)[0])
        assert np.array_equal(fine, g.refine(q, index.search(q, K * F)[0], K)[0])
    with pytest.raises(ValueError):
        nnsearch.matching_LSH_hip(K, x, q, 64, refine_rows=x[:-1])
