"""GPU: the PQ index (csrc/pq.hip, csrc/api_pq.hip) against a pure-numpy truth (tests/_pq_truth.py).  The contract is
bit-exact: ids are compared with ==, distances and table entries on their bits (view(uint32))."""
import os

import numpy as np
import pytest

from _pq_truth import adc_truth, books_of, dtable64, encode_truth, pq_truth, tie_aware_vs_reference

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pq_net.npz")


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


def _books(seed, M, Ks, L):
    return np.random.default_rng(seed).standard_normal((M, Ks, L)).astype(np.float32)


def _problem(seed, n, M, Ks, L, nq):
    """seeded codebooks, codes and queries; query 0 is the reconstruction of a gallery row (distance 0 in every book), and a
    few gallery rows are copies of others, so that exact ties occur"""
    rng = np.random.default_rng(seed)
    C = _books(seed, M, Ks, L)
    codes = rng.integers(0, Ks, size=(n, M), dtype=np.uint8)
    if n > 4:
        codes[n - 1], codes[n // 3] = codes[0], codes[n // 2]
    q = rng.standard_normal((nq, M * L)).astype(np.float32)
    q[0] = np.concatenate([C[m, codes[n // 2, m]] for m in range(M)])
    return C, codes, q


SHAPES = [(1, 2, 1), (3, 16, 5), (8, 255, 2), (16, 256, 128), (64, 256, 2), (64, 256, 64)]


@pytest.mark.parametrize("M,Ks,L", SHAPES)
def test_dtable_is_the_truth_bit_for_bit(lib, M, Ks, L):
    C = _books(M + Ks + L, M, Ks, L)
    rng = np.random.default_rng(L)
    q64 = rng.standard_normal((130, M * L))
    q64[3] = np.concatenate([C[m, m % Ks] for m in range(M)]).astype(np.float64) + 2.0 ** -30      # below float32 resolution
    q32 = q64.astype(np.float32)
    colmajor = np.asfortranarray(q32)                                   # row stride 1, column stride 130
    with lib.PQIndex.empty(C, 64) as idx:
        assert (idx.n, idx.d, idx.m, idx.ks, idx.capacity) == (0, M * L, M, Ks, 64)
        assert np.array_equal(_bits(idx.codebooks), _bits(C))
        for nq in (1, 5, 130):
            for name, q in (("f32", q32[:nq]), ("f64", q64[:nq]), ("transposed view", colmajor[:nq])):
                got = idx.dtable(q)
                assert got.dtype == np.float32 and got.shape == (nq, M, Ks)
                assert np.array_equal(_bits(got), _bits(dtable64(q, C)[1])), (name, nq)
        with pytest.raises(RuntimeError, match="finite"):
            idx.dtable(np.full((1, M * L), np.nan, np.float32))


@pytest.mark.parametrize("M,Ks,L", SHAPES)
def test_encode_is_the_float64_argmin(lib, M, Ks, L):
    C = _books(7 * M + Ks + L, M, Ks, L)
    C[0, Ks - 1] = C[0, 0]                                              # two identical codewords: the lower index wins
    rng = np.random.default_rng(M)
    x64 = rng.standard_normal((5000, M * L))
    pick = rng.integers(0, Ks, size=(70, M))
    pick[:, 0] = np.where(pick[:, 0] == Ks - 1, 0, pick[:, 0])
    pick[:3, 0] = 0
    x64[:70] = np.stack([np.concatenate([C[m, pick[i, m]] for m in range(M)]) for i in range(70)])      # exact codeword rows
    x32 = x64.astype(np.float32)
    want = encode_truth(x32, C)
    assert np.array_equal(want[:70, 1:], pick[:, 1:]) and (want[:3, 0] == 0).all()
    with lib.PQIndex.empty(C, 5100) as idx:
        for n in (1, 65, 5000):
            assert np.array_equal(idx.encode(x32[:n]), want[:n]), n
        assert np.array_equal(idx.encode(x64[:65]), encode_truth(x64[:65], C))
        assert np.array_equal(idx.encode(np.asfortranarray(x32[:65])), want[:65])
        # rows that are concatenations of codewords: their own codes, at distance 0
        ids, dist, _ = idx.search(x32[:3], 1)
        assert (ids == -1).all() and np.isinf(dist).all()               # (still empty)
        idx.add(x32[:65])
        idx.add(x64[65:100].astype(np.float64))
        assert idx.n == 100
        assert np.array_equal(idx.get_codes(), encode_truth(np.concatenate([x32[:65], x64[65:100]]), C))
        ids, dist, _ = idx.search(x32[:70], 1)
        assert (dist == 0).all()
        assert np.array_equal(idx.get_codes()[ids[:, 0]], want[:70])


# (N, M, Ks, nq, K): every value of N {1, 63, 64, 65, 257, 5000, 70001}, M {1, 3, 5, 16, 32, 64}, Ks {2, 255, 256},
# nq {1, 3, 4, 5, 9, 130}, K {1, 100, 2048}; K = N, K > N (padding) and K = 2048 beside N = 2048 / 2047.  L is 2 (3 where M = 1)
SWEEP = [
    (1, 1, 2, 1, 1), (1, 3, 255, 3, 100), (1, 16, 256, 4, 2048), (1, 64, 256, 130, 1),
    (63, 5, 2, 4, 100), (63, 32, 256, 9, 2048), (63, 1, 255, 5, 1), (63, 64, 255, 1, 63),
    (64, 3, 256, 5, 1), (64, 16, 2, 130, 100), (64, 64, 256, 3, 2048), (64, 5, 255, 9, 64),
    (65, 1, 256, 9, 100), (65, 32, 255, 1, 1), (65, 64, 2, 4, 2048), (65, 16, 256, 3, 65),
    (257, 3, 2, 130, 2048), (257, 5, 256, 1, 100), (257, 64, 255, 5, 1), (257, 32, 256, 4, 257),
    (5000, 1, 2, 3, 2048), (5000, 16, 255, 130, 100), (5000, 32, 256, 5, 1), (5000, 64, 256, 9, 100), (5000, 5, 256, 4, 2048),
    (5000, 3, 255, 1, 100),
    (70001, 16, 256, 9, 100), (70001, 1, 255, 4, 2048), (70001, 64, 256, 3, 1), (70001, 32, 2, 5, 100), (70001, 3, 256, 1, 2048),
    (70001, 5, 255, 130, 1),
    (2048, 16, 256, 3, 2048), (2047, 5, 255, 3, 2048), (100, 64, 256, 2, 100), (99, 32, 256, 2, 100),
    (5000, 64, 256, 2, 100), (5000, 64, 256, 1, 100), (5000, 32, 256, 2, 1), (5000, 16, 256, 1, 2048),
]


@pytest.mark.parametrize("n,M,Ks,nq,k", SWEEP)
def test_shape_sweep(lib, n, M, Ks, nq, k):
    L = 3 if M == 1 else 2
    C, codes, q = _problem(n * 31 + M * 7 + Ks + nq + k, n, M, Ks, L, nq)
    want = pq_truth(q, C, codes, k)
    with lib.PQIndex.from_codes(C, codes) as idx:
        assert (idx.n, idx.m, idx.ks, idx.d) == (n, M, Ks, M * L)
        ids, dist, _ = idx.search(q, k)
    assert ids.dtype == np.int64 and dist.dtype == np.float32
    assert np.array_equal(_bits(dist), _bits(want[1]))
    assert np.array_equal(ids, want[0])
    if k > n:
        assert (ids[:, n:] == -1).all() and np.isposinf(dist[:, n:]).all() and (ids[:, :n] >= 0).all()


def test_ties_identical_codes(lib):
    C = _books(1, 16, 256, 4)
    codes = np.repeat(np.random.default_rng(1).integers(0, 256, size=(1, 16), dtype=np.uint8), 5000, axis=0)
    q = np.random.default_rng(2).standard_normal((3, 64)).astype(np.float32)
    with lib.PQIndex.from_codes(C, codes) as idx:
        ids, dist, _ = idx.search(q, 100)
    assert np.array_equal(ids, np.tile(np.arange(100, dtype=np.int64), (3, 1)))
    assert _same((ids, dist), pq_truth(q, C, codes, 100))


def test_ties_two_valued_gallery(lib):
    # one book of two codewords at 0 and 1 in one dimension; even rows hold codeword 0, odd rows codeword 1.  Query 0.25: the
    # evens (0.0625) by id, then the odds (0.5625) by id; query 0.75: the other way round
    C = np.array([[[0.0], [1.0]]], np.float32)
    codes = (np.arange(1000) % 2).astype(np.uint8)[:, None]
    q = np.array([[0.25], [0.75]], np.float32)
    with lib.PQIndex.from_codes(C, codes) as idx:
        ids, dist, _ = idx.search(q, 600)
    evens, odds = np.arange(0, 1000, 2, dtype=np.int64), np.arange(1, 1000, 2, dtype=np.int64)
    assert np.array_equal(ids[0], np.concatenate([evens, odds[:100]]))
    assert np.array_equal(ids[1], np.concatenate([odds, evens[:100]]))
    assert np.array_equal(dist[0], np.concatenate([np.full(500, 0.0625, np.float32), np.full(100, 0.5625, np.float32)]))
    assert np.array_equal(dist[1], dist[0])


def test_overflowing_table_entries_are_ordinary_infinities(lib):
    C = np.ones((4, 16, 2), np.float32)
    codes = np.random.default_rng(3).integers(0, 16, size=(300, 4), dtype=np.uint8)
    q = np.full((2, 8), 3e20, np.float32)
    q[1, 2:] = 1.0                                                      # only book 0 overflows: still every distance +inf
    with lib.PQIndex.from_codes(C, codes) as idx:
        assert np.isposinf(idx.dtable(q)[:, 0]).all()
        ids, dist, _ = idx.search(q, 100)
        ids_all, dist_all, _ = idx.search(q, 512)
    assert np.array_equal(ids, np.tile(np.arange(100, dtype=np.int64), (2, 1))) and np.isposinf(dist).all()
    assert np.array_equal(ids_all[:, :300], np.tile(np.arange(300, dtype=np.int64), (2, 1))) and (ids_all[:, 300:] == -1).all()
    assert np.isposinf(dist_all).all()


def test_non_finite_host_queries_are_refused(lib):
    C, codes, q = _problem(4, 100, 3, 16, 2, 3)
    with lib.PQIndex.from_codes(C, codes) as idx:
        for bad in (np.nan, np.inf, -np.inf):
            qq = q.copy()
            qq[2, 5] = bad
            with pytest.raises(RuntimeError, match="finite"):
                idx.search(qq, 5)
        assert _same(idx.search(q, 5)[:2], pq_truth(q, C, codes, 5))


def test_allow_bitmap(lib):
    import torch
    n, k = 5000, 10
    C, codes, q = _problem(10, n, 5, 255, 2, 3)
    rng = np.random.default_rng(3)
    mask = rng.random(n) < 0.3
    some_ids = np.sort(rng.choice(n, size=200, replace=False)).astype(np.int64) + 7000
    with lib.PQIndex.from_codes(C, codes, row_offset=7000) as idx:
        plain = idx.search(q, k)[:2]
        cases = {"mask": (mask, mask), "ids": (some_ids, np.isin(np.arange(n), some_ids - 7000)),
                 "all": (np.ones(n, bool), np.ones(n, bool)), "three": (np.array([7003, 7100, 11999]), None),
                 "none": (np.zeros(n, bool), np.zeros(n, bool))}
        for name, (allow, allowed) in cases.items():
            if allowed is None:
                allowed = np.isin(np.arange(n), np.asarray(allow) - 7000)
            want = pq_truth(q, C, codes, k, row_offset=7000, allowed=allowed)
            got = idx.search(q, k, allow=allow)[:2]
            assert _same(got, want), name
            bits = lib.allow_bitmap(allow, n, 7000)
            dbits = torch.from_numpy(np.ascontiguousarray(bits).view(np.int64).copy()).to("cuda:0")
            torch.cuda.synchronize()
            assert _same(idx.search(q, k, allow_ptr=dbits.data_ptr())[:2], want), name + " (device bitmap)"
            if name == "all":
                assert _same(got, plain)
            if name == "three":
                assert (got[0][:, 3:] == -1).all() and np.isposinf(got[1][:, 3:]).all() and (got[0][:, :3] >= 7000).all()
            if name == "none":
                assert (got[0] == -1).all() and np.isposinf(got[1]).all()


def test_row_offset_and_row_stride(lib):
    C, codes, q = _problem(6, 5000, 16, 256, 2, 3)
    want = pq_truth(q, C, codes, 100, row_offset=10 ** 9)
    with lib.PQIndex.from_codes(C, codes, row_offset=10 ** 9) as idx:
        got = idx.search(q, 100)[:2]
    assert got[0].min() >= 10 ** 9 and _same(got, want)
    C, codes, q = _problem(5, 257, 5, 16, 2, 3)
    wide = np.full((257, 11), 0xA5, np.uint8)                           # what lies between the rows must not matter (>= ks too)
    wide[:, :5] = codes
    with lib.PQIndex.from_codes(C, wide[:, :5]) as idx:                 # row stride 11 bytes
        assert np.array_equal(idx.get_codes(), codes) and np.array_equal(idx.get_codes(60, 10), codes[60:70])
        assert _same(idx.search(q, 100)[:2], pq_truth(q, C, codes, 100))


def test_append(lib):
    C, codes, q = _problem(11, 300, 5, 255, 4, 5)
    rng = np.random.default_rng(12)
    x = rng.standard_normal((300, 20)).astype(np.float32)
    enc = encode_truth(x, C)
    # rows appended as codes keep their codes, rows added as vectors get the encoder's
    parts = [(0, 1, "codes"), (1, 63, "add"), (63, 64, "codes"), (64, 65, "add"), (65, 130, "codes"), (130, 300, "add")]
    full = codes.copy()
    for a, b, how in parts:
        if how == "add":
            full[a:b] = enc[a:b]
    with lib.PQIndex.from_codes(C, full) as one, lib.PQIndex.empty(C, 300) as app:
        assert (app.n, app.capacity) == (0, 300)
        ids_e, dist_e, _ = app.search(q, 4)                             # empty: all padding
        assert (ids_e == -1).all() and np.isposinf(dist_e).all()
        for a, b, how in parts:                                         # 1, 62, 1, 1, 65, 170 rows: across rows 64, 128, 192, 256
            if how == "add":
                app.add(x[a:b])
            else:
                app.append_codes(codes[a:b])
            assert app.n == b
        want = one.search(q, 100)[:2]
        assert _same(app.search(q, 100)[:2], want)
        assert np.array_equal(app.get_codes(), full) and np.array_equal(one.get_codes(), full)
        with pytest.raises(RuntimeError, match="capacity"):
            app.append_codes(codes[:1])
        with pytest.raises(RuntimeError, match="capacity"):
            app.add(x[:1])
        assert app.n == 300
        assert _same(app.search(q, 100)[:2], want)
    assert _same(want, pq_truth(q, C, full, 100))


def test_matrix_budget_chunks_give_the_same_answer(lib):
    C, codes, q = _problem(9, 5000, 16, 256, 2, 130)
    with lib.PQIndex.from_codes(C, codes) as idx:
        got0 = idx.search(q, 100)[:2]
        npad = (5000 + 63) // 64 * 64
        lib.set_global_option("pq_matrix_bytes", 50 * npad * 4)         # 130 queries: chunks of 48, 48, 34
        try:
            got1 = idx.search(q, 100)[:2]
            lib.set_global_option("pq_matrix_bytes", 1)                 # below one row: one tile of four queries per chunk
            got2 = idx.search(q[:9], 100)[:2]
        finally:
            lib.set_global_option("pq_matrix_bytes", 0)
        assert lib.get_global_option("pq_matrix_bytes") == 2 << 30
    assert _same(got0, pq_truth(q, C, codes, 100))
    assert _same(got1, got0)
    assert _same(got2, (got0[0][:9], got0[1][:9]))


def test_device_path_on_a_side_stream(lib):
    import torch
    dev = torch.device("cuda", 0)
    C, codes, q = _problem(12, 5000, 32, 256, 2, 130)
    idx = lib.PQIndex.from_codes(C, codes)
    try:
        host = {nq: idx.search(q[:nq], 100)[:2] for nq in (130, 7)}
        side = torch.cuda.Stream(device=dev)
        qh = torch.from_numpy(q * 2).pin_memory()

        def run(nq):
            out_i = torch.empty((nq, 100), dtype=torch.int64, device=dev)
            out_d = torch.empty((nq, 100), dtype=torch.float32, device=dev)
            with torch.cuda.stream(side):
                qd = (qh[:nq].to(dev, non_blocking=True) * 0.5).contiguous()      # produced on the side stream
                idx.search_device(qd.data_ptr(), nq, 100, out_i.data_ptr(), out_d.data_ptr(), stream=side.cuda_stream)
            side.synchronize()
            return out_i.cpu().numpy(), out_d.cpu().numpy()

        for order in ((130, 7), (7, 130)):                              # workspace growth both ways
            for nq in order:
                a, b = run(nq), run(nq)
                assert _same(a, b)
                assert _same(a, host[nq]), nq
            idx.close()
            idx = lib.PQIndex.from_codes(C, codes)                      # a fresh handle: the second order grows from nothing
    finally:
        idx.close()
    assert _same(host[7], pq_truth(q[:7], C, codes, 100))


def test_device_codes_are_checked_at_create_and_append(lib):
    import torch
    C, codes, q = _problem(13, 257, 5, 255, 2, 3)
    wide = np.full((257, 8), 0xFF, np.uint8)                            # row stride 8: the bytes between the rows are not codes
    wide[:, :5] = codes
    good = torch.from_numpy(wide).to("cuda:0")
    bad_host = wide.copy()
    bad_host[200, 4] = 255
    bad = torch.from_numpy(bad_host).to("cuda:0")
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match=">= ks"):
        lib.PQIndex.from_device_ptr(C, bad.data_ptr(), 257, row_stride_bytes=8)
    with lib.PQIndex.from_device_ptr(C, good.data_ptr(), 200, row_stride_bytes=8, capacity=300) as idx:
        rc = lib.load().mi_pq_append_codes(idx._h, bad.data_ptr() + 200 * 8, 57, 8, lib.MI_DEVICE)
        assert rc == lib.MI_ERR_INVALID and b">= ks" in lib.load().mi_last_error()
        assert _same(idx.search(q, 50)[:2], pq_truth(q, C, codes[:200], 50))      # the index answers as before
        lib.check(lib.load().mi_pq_append_codes(idx._h, good.data_ptr() + 200 * 8, 57, 8, lib.MI_DEVICE))
        idx.n += 57
        assert np.array_equal(idx.get_codes(), codes)
        assert _same(idx.search(q, 50)[:2], pq_truth(q, C, codes, 50))


def test_matching_pq_net_hip(lib):
    from isehr_amd.nnsearch import matching_PQ_Net_hip
    z = np.load(GOLD)
    cw, query, codes, M, K, idx_ref = z["codewords"], z["query"], z["codes"], int(z["n_books"]), int(z["K"]), z["idx"]
    idx, tpq = matching_PQ_Net_hip(K, cw, query, M, codes)
    assert idx.dtype == np.int64 and idx.shape == (7, K) and tpq > 0
    assert np.array_equal(idx, pq_truth(query, books_of(cw, M), codes, K)[0])
    assert tie_aware_vs_reference(idx_ref, idx, cw, query, M, codes) == []
    idx64, _ = matching_PQ_Net_hip(K, cw.astype(np.float64), query.astype(np.float64), M, codes.astype(np.int64))
    assert np.array_equal(idx64, idx)
