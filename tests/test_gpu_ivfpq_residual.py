"""GPU: the residual IVF-PQ index (csrc/ivfpq_residual.hip, csrc/api_ivfpq.hip) against a pure-numpy truth
(tests/_ivfpq_residual_truth.py).  The contract is bit-exact: ids are compared with ==, distances on their bits (view(uint32))."""
import numpy as np
import pytest

from _ivfpq_residual_truth import (residual_encode_truth, residual_ivfpq_truth, residual_rows_truth)
from _ivfpq_truth import probe_truth
from _pq_train_truth import rows_init, train_truth
from _pq_truth import pq_truth
from test_ivfpq_residual_cpu import QUALITY, mse, quality_fixture, quality_truth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from isehr_amd import _lib
    _lib.load()
    return _lib


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want):
    """(ids, dist) pairs equal: ids by value, distances by bits"""
    return np.array_equal(got[0], want[0]) and np.array_equal(_bits(got[1]), _bits(want[1]))


def _problem(seed, n, nlist, M, Ks, L, nq):
    """seeded centroids (spread 3, so that the residual matters), codebooks, codes, lists and queries near the centroids.  Row
    n - 1 is a copy of row 0's code in ANOTHER list and row n // 3 a copy of row n // 2 in the SAME list (an exact tie)"""
    rng = np.random.default_rng(seed)
    Cb = rng.standard_normal((M, Ks, L)).astype(np.float32)
    G = (3 * rng.standard_normal((nlist, M * L))).astype(np.float32)
    codes = rng.integers(0, Ks, size=(n, M), dtype=np.uint8)
    lists = rng.integers(0, nlist, size=n).astype(np.uint8)
    if n > 4:
        codes[n - 1], codes[n // 3] = codes[0], codes[n // 2]
        lists[n - 1], lists[n // 3] = (int(lists[0]) + 1) % nlist, lists[n // 2]
    q = (G[rng.integers(0, nlist, size=nq)] + rng.standard_normal((nq, M * L))).astype(np.float32)
    return G, Cb, codes, lists, q


@pytest.fixture(scope="module")
def big():
    """The 9000-row problem (143 blocks in 5 lists = 3 slabs of 64 virtual blocks) and its truth, shared and left unchanged."""
    G, Cb, codes, lists, q = _problem(9000, 9000, 5, 4, 16, 8, 9)
    want = residual_ivfpq_truth(q, G, Cb, codes, lists, probe_truth(q, G, 5), 100)
    for a in (G, Cb, codes, lists, q) + want:
        a.setflags(write=False)
    return G, Cb, codes, lists, q, want


# (n, nlist, nprobe, k, nq, (d, M, Ks)): the smallest index; M no multiple of 4 and padding; the real table shape; the 64 KiB LDS
# table.  The 9000-row case is test_three_slabs below
SWEEP = [(1, 2, 1, 1, 1, (8, 2, 4)), (63, 7, 3, 100, 130, (12, 3, 5)), (300, 4, 4, 10, 3, (2048, 16, 256)),
         (200, 3, 2, 5, 2, (64, 64, 256))]


@pytest.mark.parametrize("n,nlist,nprobe,k,nq,shape", SWEEP)
def test_search_is_the_truth(lib, n, nlist, nprobe, k, nq, shape):
    d, M, Ks = shape
    G, Cb, codes, lists, q = _problem(n + nlist, n, nlist, M, Ks, d // M, nq)
    probes = probe_truth(q, G, nprobe)
    want = residual_ivfpq_truth(q, G, Cb, codes, lists, probes, k, row_offset=1000)
    with lib.IVFPQIndex.from_codes(G, Cb, codes, lists, row_offset=1000, by_residual=True) as idx:
        assert idx.by_residual and (idx.n, idx.m, idx.ks, idx.d, idx.nlist) == (n, M, Ks, d, nlist)
        assert np.array_equal(idx.probe(q, nprobe), probes)
        before = idx.hbm_bytes
        ids, dist, _ = idx.search(q, k, nprobe=nprobe)
        assert idx.hbm_bytes >= before + nprobe * M * Ks * 4            # the table buffer is counted
        stored = idx.get_rows()
    assert np.array_equal(stored[0], codes) and np.array_equal(stored[1], lists)          # residual codes are stored as given
    assert np.array_equal(_bits(dist), _bits(want[1]))
    assert np.array_equal(ids, want[0])


@pytest.mark.parametrize("n,nlist,nprobe,k,nq,shape", SWEEP[1:3])
def test_float64_queries(lib, n, nlist, nprobe, k, nq, shape):
    """float64 queries keep their low bits: the residual is double(x) - double(G[l]) of the float64 value"""
    d, M, Ks = shape
    G, Cb, codes, lists, q32 = _problem(n + nlist, n, nlist, M, Ks, d // M, nq)
    q = q32.astype(np.float64) + 2.0 ** -30 * np.random.default_rng(n).standard_normal(q32.shape)
    assert not np.array_equal(q, q.astype(np.float32))
    with lib.IVFPQIndex.from_codes(G, Cb, codes, lists, by_residual=True) as idx:
        for name, qq in (("contiguous", q), ("transposed view", np.asfortranarray(q))):
            got = idx.search(qq, k, nprobe=nprobe)[:2]
            assert _same(got, residual_ivfpq_truth(q, G, Cb, codes, lists, probe_truth(q, G, nprobe), k)), name


def test_three_slabs(lib, big):
    G, Cb, codes, lists, q, want = big
    blocks = (np.bincount(lists, minlength=5) + 63) // 64
    assert blocks.sum() > 128 and (np.cumsum(blocks) % 64 != 0).all()     # 3 slabs; no list ends on a slab boundary
    with lib.IVFPQIndex.from_codes(G, Cb, codes, lists, by_residual=True) as idx:
        assert _same(idx.search(q, 100, nprobe=5)[:2], want)
        for nprobe in (1, 3):
            assert _same(idx.search(q, 100, nprobe=nprobe)[:2],
                         residual_ivfpq_truth(q, G, Cb, codes, lists, probe_truth(q, G, nprobe), 100)), nprobe


def test_chunking_does_not_change_the_bits(lib, big):
    G, Cb, codes, lists, q, want = big
    with lib.IVFPQIndex.from_codes(G, Cb, codes, lists, by_residual=True) as idx:
        try:
            # one query takes 3 slabs * 100 keys * 8 bytes + 5 tables * 64 entries * 4 bytes = 3680 bytes: one query per chunk
            lib.set_global_option("pq_matrix_bytes", 4000)
            one = idx.search(q, 100, nprobe=5)[:2]
            lib.set_global_option("pq_matrix_bytes", 3 * 3680 + 100)                      # three queries per chunk
            three = idx.search(q, 100, nprobe=5)[:2]
        finally:
            lib.set_global_option("pq_matrix_bytes", 0)
        assert lib.get_global_option("pq_matrix_bytes") == 2 << 30
    assert _same(one, want) and _same(three, want)


def test_same_code_in_different_lists(lib):
    G, Cb, codes, lists, q = _problem(77, 40, 3, 4, 16, 2, 3)
    codes[11], lists[11], lists[30] = codes[30], 0, 2
    pr = np.tile(np.arange(3), (q.shape[0], 1))
    want = residual_ivfpq_truth(q, G, Cb, codes, lists, pr, 40)
    with lib.IVFPQIndex.from_codes(G, Cb, codes, lists, by_residual=True) as idx:
        ids, dist, _ = idx.search(q, 40, probes=pr)
    assert _same((ids, dist), want)
    for i in range(q.shape[0]):
        d = dict(zip(ids[i].tolist(), dist[i].tolist()))
        assert d[11] != d[30]


def test_zero_centroids_are_the_plain_index(lib):
    G, Cb, codes, lists, q = _problem(5, 5000, 7, 6, 16, 2, 5)
    Z = np.zeros_like(G)
    with lib.IVFPQIndex.from_codes(Z, Cb, codes, lists, by_residual=True) as res, \
            lib.IVFPQIndex.from_codes(Z, Cb, codes, lists) as plain, lib.PQIndex.from_codes(Cb, codes) as flat:
        assert res.by_residual and not plain.by_residual
        rng = np.random.default_rng(6)
        for nprobe in (1, 3, 7):
            pr = np.stack([rng.permutation(7)[:nprobe] for _ in range(q.shape[0])])        # the zero centroids all tie
            assert _same(res.search(q, 100, probes=pr)[:2], plain.search(q, 100, probes=pr)[:2]), nprobe
            assert _same(res.search(q, 100, nprobe=nprobe)[:2], plain.search(q, 100, nprobe=nprobe)[:2]), nprobe
        assert _same(res.search(q, 100, nprobe=7)[:2], flat.search(q, 100)[:2])
        assert _same(res.search(q, 100, nprobe=7)[:2], pq_truth(q, Cb, codes, 100))


def test_add_encodes_the_residual(lib):
    import torch
    rng = np.random.default_rng(8)
    M, Ks, L, nlist, n = 3, 16, 4, 5, 300
    d = M * L
    G = (3 * rng.standard_normal((nlist, d))).astype(np.float32)
    Cb = rng.standard_normal((M, Ks, L)).astype(np.float32)
    x64 = G[rng.integers(0, nlist, size=n)] + rng.standard_normal((n, d))
    x32 = x64.astype(np.float32)
    wide = np.zeros((n, 2 * d + 3), np.float32)                           # rows with a row stride and a column stride
    wide[:, 1:2 * d:2] = x32
    for name, rows, truth_of in (("f32", x32, x32), ("f64", x64, x64), ("strided", wide[:, 1:2 * d:2], x32),
                                 ("transposed view", np.asfortranarray(x64), x64)):
        codes, lists = residual_encode_truth(truth_of, G, Cb)
        with lib.IVFPQIndex.empty(G, Cb, n, by_residual=True) as idx:
            idx.add(rows[:130])
            idx.add(rows[130:])
            got = idx.get_rows()
            assert np.array_equal(got[1], lists) and np.array_equal(got[0], codes), name
            assert np.array_equal(_bits(idx.residual_rows(rows)), _bits(residual_rows_truth(truth_of, G, lists))), name
            other = (lists.astype(np.int64) + 1) % nlist
            assert np.array_equal(_bits(idx.residual_rows(rows, other)), _bits(residual_rows_truth(truth_of, G, other))), name
    codes, lists = residual_encode_truth(x32, G, Cb)
    xd = torch.from_numpy(x32).to("cuda:0")
    torch.cuda.synchronize()
    with lib.IVFPQIndex.empty(G, Cb, n, by_residual=True) as idx, lib.IVFPQIndex.empty(G, Cb, n) as plain:
        idx.add_device(xd.data_ptr(), n)
        got = idx.get_rows()
        assert np.array_equal(got[1], lists) and np.array_equal(got[0], codes)
        q = x32[:7]
        pr = probe_truth(q, G, 2)
        assert _same(idx.search(q, 20, nprobe=2)[:2], residual_ivfpq_truth(q, G, Cb, codes, lists, pr, 20))
        # residual_rows does not depend on the kind of the index
        assert np.array_equal(_bits(plain.residual_rows(x32)), _bits(residual_rows_truth(x32, G, lists)))
        # device rows with a row and a column stride, lists assigned or given on the device, into a device buffer
        call = lib.load().mi_ivfpq_residual_rows
        wd = torch.from_numpy(wide).to("cuda:0")
        od = torch.zeros((n, d), dtype=torch.float32, device="cuda:0")
        other = ((lists.astype(np.int64) + 2) % nlist).astype(np.uint8)
        ld = torch.from_numpy(other).to("cuda:0")
        torch.cuda.synchronize()
        first = wd.data_ptr() + 4                                                         # element (0, 1) of `wide`
        lib.check(call(idx._h, first, n, lib.MI_F32, wide.shape[1], 2, lib.MI_DEVICE, None, od.data_ptr(), lib.MI_DEVICE))
        assert np.array_equal(_bits(od.cpu().numpy()), _bits(residual_rows_truth(x32, G, lists)))
        lib.check(call(idx._h, first, n, lib.MI_F32, wide.shape[1], 2, lib.MI_DEVICE, ld.data_ptr(), od.data_ptr(), lib.MI_DEVICE))
        assert np.array_equal(_bits(od.cpu().numpy()), _bits(residual_rows_truth(x32, G, other)))
        host_out = np.zeros((n, d), np.float32)
        lib.check(call(idx._h, first, n, lib.MI_F32, wide.shape[1], 2, lib.MI_DEVICE, ld.data_ptr(), host_out.ctypes.data, lib.MI_HOST))
        assert np.array_equal(_bits(host_out), _bits(residual_rows_truth(x32, G, other)))
        wrong = other.copy()
        wrong[n - 1] = nlist
        wrongd = torch.from_numpy(wrong).to("cuda:0")
        torch.cuda.synchronize()
        for _ in range(2):                                                                # the flag is put back after a refusal
            assert call(idx._h, first, n, lib.MI_F32, wide.shape[1], 2, lib.MI_DEVICE, wrongd.data_ptr(), od.data_ptr(),
                        lib.MI_DEVICE) == lib.MI_ERR_INVALID
            assert b">= nlist" in lib.load().mi_last_error()
        lib.check(call(idx._h, first, n, lib.MI_F32, wide.shape[1], 2, lib.MI_DEVICE, ld.data_ptr(), od.data_ptr(), lib.MI_DEVICE))
        bad, out = np.array([0, nlist], np.uint8), np.zeros((2, d), np.float32)           # past the wrapper's own check
        with pytest.raises(RuntimeError, match=">= nlist"):
            lib.check(lib.load().mi_ivfpq_residual_rows(idx._h, x32.ctypes.data, 2, lib.MI_F32, d, 1, lib.MI_HOST, bad.ctypes.data,
                                                        out.ctypes.data, lib.MI_HOST))


def _device_search(torch, idx, q, k, nprobe, probes=None, allow=None, stream=None):
    dev = torch.device("cuda", 0)
    nq = q.shape[0]
    out_i = torch.empty((nq, k), dtype=torch.int64, device=dev)
    out_d = torch.empty((nq, k), dtype=torch.float32, device=dev)
    qd = torch.from_numpy(np.array(q, np.float32)).to(dev)
    pd = None if probes is None else torch.from_numpy(np.ascontiguousarray(probes, np.int32)).to(dev)
    torch.cuda.synchronize()
    idx.search_device(qd.data_ptr(), nq, k, out_i.data_ptr(), out_d.data_ptr(), nprobe=nprobe,
                      probes_ptr=None if pd is None else pd.data_ptr(), allow_ptr=None if allow is None else allow.data_ptr(),
                      stream=None if stream is None else stream.cuda_stream)
    (torch.cuda.current_stream() if stream is None else stream).synchronize()
    torch.cuda.synchronize()
    return out_i.cpu().numpy(), out_d.cpu().numpy()


def test_explicit_probes_bitmaps_and_padding(lib):
    import torch
    G, Cb, codes, lists, q = _problem(40, 700, 7, 5, 16, 2, 5)
    lists[lists == 4] = 3                                                 # list 4 is empty
    pr = np.array([[0, 1, 2, 3], [6, -1, 6, 6], [-1, -1, -1, -1], [5, 4, 5, -1], [4, 4, -1, 4]], np.int32)
    allowed = np.random.default_rng(41).random(700) < 0.5
    with lib.IVFPQIndex.from_codes(G, Cb, codes, lists, row_offset=3, by_residual=True) as idx:
        want = residual_ivfpq_truth(q, G, Cb, codes, lists, pr, 300, row_offset=3)
        host = idx.search(q, 300, probes=pr)[:2]
        assert _same(host, want)
        assert (host[0][2] == -1).all() and np.isposinf(host[1][2]).all()         # no list at all
        assert (host[0][4] == -1).all()                                           # an empty list
        found = (want[0] >= 0).sum(1)
        assert 0 < found[1] < 300 and (host[0][1][found[1]:] == -1).all() and np.isposinf(host[1][1][found[1]:]).all()   # padding
        assert _same(_device_search(torch, idx, q, 300, 4, pr), want)
        wild = pr.copy()
        wild[1, 1], wild[2, 0], wild[2, 3] = 7, 2 ** 31 - 1, -5                   # on the device out of range acts as -1
        assert _same(_device_search(torch, idx, q, 300, 4, wild), want)
        # allow bitmaps, host and device
        want_allow = residual_ivfpq_truth(q, G, Cb, codes, lists, pr, 300, row_offset=3, allowed=allowed)
        assert _same(idx.search(q, 300, probes=pr, allow=allowed)[:2], want_allow)
        words = torch.from_numpy(np.asarray(lib.allow_bitmap(allowed, 700, 0)).view(np.int64).copy()).to("cuda:0")
        torch.cuda.synchronize()
        assert _same(idx.search(q, 300, probes=pr, allow_ptr=words.data_ptr())[:2], want_allow)
        assert _same(_device_search(torch, idx, q, 300, 4, pr, allow=words), want_allow)
        want3 = residual_ivfpq_truth(q, G, Cb, codes, lists, probe_truth(q, G, 3), 300, row_offset=3, allowed=allowed)
        assert _same(idx.search(q, 300, nprobe=3, allow=allowed)[:2], want3)


def test_appends_in_two_orders_answer_identically(lib):
    G, Cb, codes, lists, q = _problem(50, 3000, 7, 4, 16, 2, 5)
    pr = probe_truth(q, G, 3)
    want = residual_ivfpq_truth(q, G, Cb, codes, lists, pr, 500)
    order = np.random.default_rng(51).permutation(3000)
    with lib.IVFPQIndex.empty(G, Cb, 3000, by_residual=True) as fwd, lib.IVFPQIndex.empty(G, Cb, 3000, by_residual=True) as steps:
        fwd.append_codes(codes, lists)
        for a, b in ((0, 1), (1, 700), (700, 764), (764, 3000)):
            steps.append_codes(codes[a:b], lists[a:b])
        assert _same(fwd.search(q, 500, nprobe=3)[:2], want)
        assert _same(steps.search(q, 500, nprobe=3)[:2], want)
    # the rows in another order: other ids, the same (distance, original row) pairs
    with lib.IVFPQIndex.from_codes(G, Cb, codes[order], lists[order], by_residual=True) as shuffled:
        ids, dist, _ = shuffled.search(q, 500, nprobe=3)
    back = np.where(ids >= 0, order[np.maximum(ids, 0)], -1)
    for i in range(q.shape[0]):
        resort = np.lexsort((back[i], dist[i]))
        assert np.array_equal(back[i][resort], want[0][i]) and np.array_equal(_bits(dist[i][resort]), _bits(want[1][i]))


def test_device_path_on_a_side_stream(lib, big):
    import torch
    G, Cb, codes, lists, q, want = big
    side = torch.cuda.Stream(device=torch.device("cuda", 0))
    with lib.IVFPQIndex.from_codes(G, Cb, codes, lists, by_residual=True) as idx:
        first = _device_search(torch, idx, q, 100, 5, stream=side)
        second = _device_search(torch, idx, q, 100, 5, stream=side)
        assert _same(first, want) and _same(second, want)
        assert _same(_device_search(torch, idx, q[:4], 100, 5, stream=side), (want[0][:4], want[1][:4]))


def test_measured_stages_answer_like_search_device(lib, big):
    """mi_ivfpq_search_stages_device on both kinds of index: the ids and distance bits of search_device, times finite and >= 0,
    with pq_matrix_bytes so low that the times are sums over several chunks"""
    import torch
    G, Cb, codes, lists, q, want = big
    dev = torch.device("cuda", 0)
    qd = torch.from_numpy(np.array(q, np.float32)).to(dev)
    nq, k = q.shape[0], 100
    with lib.IVFPQIndex.from_codes(G, Cb, codes, lists, by_residual=True) as res, lib.IVFPQIndex.from_codes(G, Cb, codes, lists) as plain:
        for name, idx in (("residual", res), ("plain", plain)):
            ref = _device_search(torch, idx, q, k, 5)
            if name == "residual":
                assert _same(ref, want)
            for budget in (0, 2 * 3680 + 100):                                            # one chunk; two or three queries per chunk
                out_i = torch.full((nq, k), -7, dtype=torch.int64, device=dev)
                out_d = torch.full((nq, k), -7.0, dtype=torch.float32, device=dev)
                torch.cuda.synchronize()
                try:
                    lib.set_global_option("pq_matrix_bytes", budget)
                    table_ms, scan_ms = idx.search_stages_device(qd.data_ptr(), nq, k, out_i.data_ptr(), out_d.data_ptr(), nprobe=5,
                                                                 stream=torch.cuda.current_stream().cuda_stream)
                finally:
                    lib.set_global_option("pq_matrix_bytes", 0)
                torch.cuda.synchronize()
                assert _same((out_i.cpu().numpy(), out_d.cpu().numpy()), ref), (name, budget)
                assert np.isfinite([table_ms, scan_ms]).all() and table_ms >= 0.0 and scan_ms >= 0.0, (name, budget, table_ms, scan_ms)
                assert table_ms + scan_ms > 0.0, (name, budget)
        t, u = res.search_stages_device(qd.data_ptr(), 0, k, 0, nprobe=5)
        assert (t, u) == (0.0, 0.0)
        with pytest.raises(RuntimeError, match="nprobe must"):
            res.search_stages_device(qd.data_ptr(), nq, k, 16, nprobe=6)


def test_a_far_centroid_gives_infinite_distances(lib):
    G, Cb, codes, lists, q = _problem(60, 400, 4, 4, 16, 2, 5)
    G[2] = 1e30                                                           # (x - 1e30)^2 = 1e60 overflows float32: every entry +inf
    pr = np.tile(np.array([2, 0], np.int32), (q.shape[0], 1))
    want = residual_ivfpq_truth(q, G, Cb, codes, lists, pr, 400)
    n0, n2 = int((lists == 0).sum()), int((lists == 2).sum())
    assert np.isfinite(want[1][:, :n0]).all() and np.isposinf(want[1][:, n0:]).all()
    assert np.array_equal(want[0][0][n0:n0 + n2], np.flatnonzero(lists == 2))             # behind the finite ones, by id
    with lib.IVFPQIndex.from_codes(G, Cb, codes, lists, by_residual=True) as idx:
        assert _same(idx.search(q, 400, probes=pr)[:2], want)


def test_fit_by_residual(lib):
    """Quality condition on RandomState(100) (the first draw satisfies it for the truth: test_ivfpq_residual_cpu): the residual
    index reconstructs strictly better than IVFPQIndex.fit without residuals.  The truth gives 1.954754 against 7.130240."""
    x = quality_fixture(0)
    n = x.shape[0]
    nlist, M, Ks, seed = (QUALITY[key] for key in ("nlist", "M", "Ks", "seed"))
    G, plain_t, resid_t = quality_truth(x, **QUALITY)
    with lib.IVFPQIndex.fit(x, by_residual=True, **QUALITY) as idx, lib.IVFPQIndex.fit(x, **QUALITY) as plain:
        assert idx.by_residual and not plain.by_residual and idx.n == n
        assert np.array_equal(_bits(idx.coarse), _bits(G)) and np.array_equal(_bits(plain.coarse), _bits(G))
        # the codebooks: the training truth on the float32 residual rows with the same initial rows
        codes, lists = idx.get_rows()
        assert np.array_equal(lists, resid_t[2])
        res = residual_rows_truth(x, G, lists)
        rng = np.random.RandomState(seed)
        rows = np.stack([rng.choice(n, Ks, replace=False) for _ in range(M)])
        Cr, moved = train_truth(res, M, Ks, 20, rows_init(res, M, rows))
        assert np.array_equal(_bits(idx.codebooks), _bits(Cr)) and np.array_equal(idx.train_moved, moved)
        assert np.array_equal(_bits(Cr), _bits(resid_t[0])) and np.array_equal(codes, resid_t[1])
        # the index answers as the truth given those codebooks
        q = x[:9] + np.float32(0.01)
        for nprobe in (2, 8):
            pr = probe_truth(q, G, nprobe)
            assert _same(idx.search(q, 10, nprobe=nprobe)[:2], residual_ivfpq_truth(q, G, Cr, codes, lists, pr, 10)), nprobe
        pcodes, plists = plain.get_rows()
        e_resid, e_plain = mse(x, idx.coarse, idx.codebooks, codes, lists, True), mse(x, plain.coarse, plain.codebooks, pcodes, plists, False)
        print("mean squared reconstruction error: plain %.6f residual %.6f" % (e_plain, e_resid))
        assert e_resid < e_plain


def test_ann(lib):
    from isehr_amd.knn import ANN, KNN
    rng = np.random.RandomState(3)
    n, d, nc = 1500, 16, 6
    cen = rng.randn(nc, d) * 3
    db = np.float32(cen[rng.randint(nc, size=n)] + 0.3 * rng.randn(n, d))
    q = np.float32(cen[rng.randint(nc, size=7)] + 0.3 * rng.randn(7, d))
    for method, prep in (("euclidean", lambda a: a), ("cosine", lambda a: (a / np.sqrt((a.astype(np.float64) ** 2).sum(1, keepdims=True)))
                                                      .astype(np.float32))):
        ann = ANN(db, method, M=4, nlist=6, nprobe=2, seed=1)
        try:
            idx = ann.index
            assert idx.by_residual and idx.n == n and (idx.m, idx.ks, idx.nlist) == (4, 256, 6)
            codes, lists = idx.get_rows()
            dist, ids = ann.search(q, 10)
            assert dist.dtype == np.float32 and ids.dtype == np.int64 and dist.shape == ids.shape == (7, 10)
            want = residual_ivfpq_truth(prep(q), idx.coarse, idx.codebooks, codes, lists, probe_truth(prep(q), idx.coarse, 2), 10)
            assert _same((ids, dist), want), method
            got_codes, got_lists = residual_encode_truth(prep(db), idx.coarse, idx.codebooks)
            assert np.array_equal(codes, got_codes) and np.array_equal(lists, got_lists), method
            assert (np.diff(dist, axis=1) >= 0).all()
        finally:
            ann.close()
    for kwargs, word in ((dict(M=65), "M = 65"), (dict(nlist=257), "nlist = 257"), (dict(nbits=4), "nbits = 4")):
        with pytest.raises(ValueError, match=word):
            ANN(db, **kwargs)
    assert KNN is not ANN
