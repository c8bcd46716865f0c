"""GPU: the binary index (csrc/hamming.hip, csrc/api_hamming.hip) against a pure-numpy truth (tests/_hamming_truth.py).  Integer
results, compared with ==: ids and distances by (distance asc, id asc), ties at the K-th distance to the lowest ids."""
import os

import numpy as np
import pytest

from _hamming_truth import INT32_MAX, greedyhash_restated, hamming_truth, tie_aware_equal

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "greedyhash.npz")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from isehr_amd import _lib
    _lib.load()
    return _lib


def _codes(seed, n, nbits, nq):
    """seeded codes; a few queries are gallery rows or near copies, so that distance 0 and small distances occur"""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 256, size=(n, nbits // 8), dtype=np.uint8)
    q = rng.integers(0, 256, size=(nq, nbits // 8), dtype=np.uint8)
    q[0] = g[n // 2]
    if nq > 2:
        q[2] = g[n - 1]
        q[2, 0] ^= 1
    return g, q


# (nbits, N, Q, K) -- every value of nbits {8, 64, 72, 2048, 4096}, N {1, 63, 64, 65, 257, 5000, 70001}, Q {1, 3, 64, 65, 130},
# K {1, 100, 2048}; K = N, K = N + 1 and K > N (padding) at both ends of K's range
SWEEP = [
    (8, 1, 1, 1), (8, 1, 3, 100), (8, 63, 64, 100), (8, 64, 65, 1), (8, 65, 130, 100), (8, 257, 3, 2048), (8, 5000, 64, 2048),
    (8, 70001, 3, 100),
    (64, 1, 65, 1), (64, 63, 1, 100), (64, 64, 3, 100), (64, 65, 64, 2048), (64, 257, 130, 100), (64, 5000, 65, 1),
    (64, 70001, 1, 2048),
    (72, 1, 130, 2048), (72, 63, 3, 1), (72, 64, 64, 100), (72, 65, 1, 100), (72, 257, 65, 2048), (72, 5000, 130, 100),
    (72, 70001, 64, 1),
    (2048, 1, 64, 100), (2048, 63, 65, 2048), (2048, 64, 130, 1), (2048, 65, 3, 100), (2048, 257, 1, 1), (2048, 5000, 3, 2048),
    (2048, 70001, 65, 100),
    (4096, 1, 1, 2048), (4096, 63, 130, 100), (4096, 64, 1, 1), (4096, 65, 65, 100), (4096, 257, 64, 2048), (4096, 5000, 1, 100),
    (4096, 70001, 3, 1),
    (64, 100, 3, 100), (64, 99, 3, 100), (72, 2048, 3, 2048), (72, 2047, 3, 2048),
]


@pytest.mark.parametrize("nbits,n,nq,k", SWEEP)
def test_shape_sweep(lib, nbits, n, nq, k):
    g, q = _codes(nbits * 7 + n + nq + k, n, nbits, nq)
    ids_t, dist_t, _ = hamming_truth(g, q, k)
    idx = lib.BinaryGallery.from_host(g)
    try:
        assert (idx.n, idx.nbits) == (n, nbits)
        ids, dist, _ = idx.search(q, k)
    finally:
        idx.close()
    assert ids.dtype == np.int64 and dist.dtype == np.int32
    assert np.array_equal(dist, dist_t)
    assert np.array_equal(ids, ids_t)
    if k > n:
        assert (ids[:, n:] == -1).all() and (dist[:, n:] == INT32_MAX).all()


def test_row_stride_and_row_offset(lib):
    g, q = _codes(5, 257, 2048, 3)
    wide = np.zeros((257, 300), np.uint8)
    wide[:] = 0xA5                                        # what lies between the rows must not matter
    wide[:, :256] = g
    qwide = np.full((3, 261), 0x5A, np.uint8)
    qwide[:, :256] = q
    ids_t, dist_t, _ = hamming_truth(g, q, 100)
    idx = lib.BinaryGallery.from_host(wide[:, :256])      # row stride 300 bytes
    try:
        ids, dist, _ = idx.search(qwide[:, :256], 100)    # query row stride 261 bytes
        assert np.array_equal(idx.get_codes(), g)
    finally:
        idx.close()
    assert np.array_equal(ids, ids_t) and np.array_equal(dist, dist_t)
    g, q = _codes(6, 5000, 64, 3)
    ids_t, dist_t, _ = hamming_truth(g, q, 100, row_offset=10 ** 9)
    idx = lib.BinaryGallery.from_host(g, row_offset=10 ** 9)
    try:
        ids, dist, _ = idx.search(q, 100)
    finally:
        idx.close()
    assert ids.min() >= 10 ** 9
    assert np.array_equal(ids, ids_t) and np.array_equal(dist, dist_t)


def test_ties_identical_rows(lib):
    nbits = 2048
    row = np.random.default_rng(1).integers(0, 256, size=nbits // 8, dtype=np.uint8)
    g = np.repeat(row[None, :], 5000, axis=0)
    q = np.stack([row, ~row])
    idx = lib.BinaryGallery.from_host(g)
    try:
        ids, dist, _ = idx.search(q, 100)
    finally:
        idx.close()
    assert np.array_equal(ids, np.tile(np.arange(100, dtype=np.int64), (2, 1)))
    assert (dist[0] == 0).all() and (dist[1] == nbits).all()


def test_ties_two_valued_gallery(lib):
    # even rows are all zeros, odd rows have their first 3 bits set.  Query = zeros: the evens at distance 0 by id, then the odds
    # at distance 3 by id.  Query = first 3 bits: the other way round
    g = np.zeros((1000, 8), np.uint8)
    g[1::2, 0] = 0b111
    q = np.zeros((2, 8), np.uint8)
    q[1, 0] = 0b111
    idx = lib.BinaryGallery.from_host(g)
    try:
        ids, dist, _ = idx.search(q, 600)
    finally:
        idx.close()
    evens, odds = np.arange(0, 1000, 2, dtype=np.int64), np.arange(1, 1000, 2, dtype=np.int64)
    assert np.array_equal(ids[0], np.concatenate([evens, odds[:100]]))
    assert np.array_equal(ids[1], np.concatenate([odds, evens[:100]]))
    assert np.array_equal(dist[0], np.concatenate([np.zeros(500, np.int32), np.full(100, 3, np.int32)]))
    assert np.array_equal(dist[1], dist[0])


def test_top_bin_4096(lib):
    g = np.full((300, 512), 0xFF, np.uint8)
    q = np.zeros((1, 512), np.uint8)
    idx = lib.BinaryGallery.from_host(g)
    try:
        ids, dist, _ = idx.search(q, 100)
    finally:
        idx.close()
    assert np.array_equal(ids[0], np.arange(100, dtype=np.int64)) and (dist == 4096).all()


def test_random_2048_bit_codes_exercise_the_lowest_id_rule(lib):
    """Uniform random 2048-bit codes put the K-th of 200 003 distances 3.3 sigma below the mean, where a few dozen rows at most share a
    distance: more rows AT the K-th distance than places left for them (asserted), but not more than K.  The second gallery --
    random codes that differ from one base row in 20 bit positions only -- has more than K rows at the K-th distance (asserted),
    so that a tie class larger than the whole answer is cut by id as well."""
    n, nq, k = 200003, 70, 100
    rng = np.random.default_rng(77)
    g = rng.integers(0, 256, size=(n, 256), dtype=np.uint8)
    q = rng.integers(0, 256, size=(nq, 256), dtype=np.uint8)
    ids_t, dist_t, full = hamming_truth(g, q, k)
    at_kth = (full == dist_t[:, -1:]).sum(axis=1)
    below = (full < dist_t[:, -1:]).sum(axis=1)
    print("rows at the K-th distance: max %d, places left for them: min %d" % (at_kth.max(), (k - below).min()))
    assert (at_kth > k - below).any(), "no query has more rows at the K-th distance than places for them"
    idx = lib.BinaryGallery.from_host(g)
    try:
        ids, dist, _ = idx.search(q, k)
    finally:
        idx.close()
    assert np.array_equal(dist, dist_t)
    assert np.array_equal(ids, ids_t)
    # more than K rows at the K-th distance
    base = rng.integers(0, 256, size=256, dtype=np.uint8)
    pos = rng.choice(2048, size=20, replace=False)
    flips = np.zeros((n, 2048), np.uint8)
    flips[:, pos] = rng.integers(0, 2, size=(n, 20), dtype=np.uint8)
    g2 = np.packbits(flips, axis=1, bitorder="little") ^ base[None, :]
    q2 = np.stack([base, g2[5], ~base])
    ids_t, dist_t, full = hamming_truth(g2, q2, k)
    at_kth = (full == dist_t[:, -1:]).sum(axis=1)
    print("second gallery, rows at the K-th distance:", at_kth.tolist())
    assert (at_kth > k).any(), "no query has more than K rows at the K-th distance"
    idx = lib.BinaryGallery.from_host(g2)
    try:
        ids, dist, _ = idx.search(q2, k)
    finally:
        idx.close()
    assert np.array_equal(dist, dist_t)
    assert np.array_equal(ids, ids_t)


def test_matrix_budget_chunks_give_the_same_answer(lib):
    g, q = _codes(9, 5000, 72, 130)
    idx = lib.BinaryGallery.from_host(g)
    try:
        ids0, dist0, _ = idx.search(q, 100)
        npad = (5000 + 63) // 64 * 64
        lib.set_global_option("hamming_matrix_bytes", 50 * npad * 2)      # 130 queries: chunks of 50, 50, 30
        try:
            ids1, dist1, _ = idx.search(q, 100)
            lib.set_global_option("hamming_matrix_bytes", 1)             # below one row: one query per chunk
            ids2, dist2, _ = idx.search(q[:5], 100)
        finally:
            lib.set_global_option("hamming_matrix_bytes", 0)
        assert lib.get_global_option("hamming_matrix_bytes") == 2 << 30
    finally:
        idx.close()
    ids_t, dist_t, _ = hamming_truth(g, q, 100)
    assert np.array_equal(ids0, ids_t) and np.array_equal(dist0, dist_t)
    assert np.array_equal(ids1, ids0) and np.array_equal(dist1, dist0)
    assert np.array_equal(ids2, ids0[:5]) and np.array_equal(dist2, dist0[:5])


def test_allow_bitmap(lib):
    import torch
    n, k = 5000, 10
    g, q = _codes(10, n, 64, 3)
    rng = np.random.default_rng(3)
    mask = rng.random(n) < 0.3
    some_ids = np.sort(rng.choice(n, size=200, replace=False)).astype(np.int64) + 7000
    idx = lib.BinaryGallery.from_host(g, row_offset=7000)
    try:
        plain = idx.search(q, k)[:2]
        cases = {"mask": (mask, mask), "ids": (some_ids, np.isin(np.arange(n), some_ids - 7000)),
                 "all": (np.ones(n, bool), np.ones(n, bool)), "three": (np.array([7003, 7100, 11999]), None),
                 "none": (np.zeros(n, bool), np.zeros(n, bool))}
        for name, (allow, allowed) in cases.items():
            if allowed is None:
                allowed = np.isin(np.arange(n), np.asarray(allow) - 7000)
            ids_t, dist_t, _ = hamming_truth(g, q, k, row_offset=7000, allowed=allowed)
            ids, dist, _ = idx.search(q, k, allow=allow)
            assert np.array_equal(ids, ids_t) and np.array_equal(dist, dist_t), name
            bits = lib.allow_bitmap(allow, n, 7000)
            dbits = torch.from_numpy(np.ascontiguousarray(bits).view(np.int64).copy()).to("cuda:0")
            torch.cuda.synchronize()
            ids_d, dist_d, _ = idx.search(q, k, allow_ptr=dbits.data_ptr())
            assert np.array_equal(ids_d, ids_t) and np.array_equal(dist_d, dist_t), name + " (device bitmap)"
            if name == "all":
                assert np.array_equal(ids, plain[0]) and np.array_equal(dist, plain[1])
            if name == "three":
                assert (ids[:, 3:] == -1).all() and (dist[:, 3:] == INT32_MAX).all() and (ids[:, :3] >= 7000).all()
            if name == "none":
                assert (ids == -1).all() and (dist == INT32_MAX).all()
    finally:
        idx.close()


def test_append(lib):
    g, q = _codes(11, 187, 72, 5)
    one = lib.BinaryGallery.from_host(g)
    app = lib.BinaryGallery.empty(300, 72)
    try:
        assert (app.n, app.nbits, app.capacity) == (0, 72, 300)
        ids_e, dist_e, _ = app.search(q, 4)                          # empty: all padding
        assert (ids_e == -1).all() and (dist_e == INT32_MAX).all()
        for a, b in ((0, 50), (50, 150), (150, 187)):                # 50, 100, 37 rows: across rows 64 and 128
            app.append(g[a:b])
        assert app.n == 187
        want = one.search(q, 100)[:2]
        got = app.search(q, 100)[:2]
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert np.array_equal(app.get_codes(), g) and np.array_equal(app.get_codes(60, 10), g[60:70])
        with pytest.raises(RuntimeError, match="capacity"):
            app.append(np.zeros((200, 9), np.uint8))
        assert app.n == 187
        again = app.search(q, 100)[:2]
        assert np.array_equal(again[0], want[0]) and np.array_equal(again[1], want[1])
    finally:
        one.close()
        app.close()
    ids_t, dist_t, _ = hamming_truth(g, q, 100)
    assert np.array_equal(want[0], ids_t) and np.array_equal(want[1], dist_t)


def test_device_path_on_a_side_stream(lib):
    import torch
    dev = torch.device("cuda", 0)
    g, q = _codes(12, 5000, 2048, 130)
    idx = lib.BinaryGallery.from_host(g)
    try:
        host = {nq: idx.search(q[:nq], 100)[:2] for nq in (130, 7)}
        side = torch.cuda.Stream(device=dev)
        qh = torch.from_numpy(q ^ 0xFF).pin_memory()

        def run(nq):
            out_i = torch.empty((nq, 100), dtype=torch.int64, device=dev)
            out_d = torch.empty((nq, 100), dtype=torch.int32, device=dev)
            with torch.cuda.stream(side):
                qd = qh[:nq].to(dev, non_blocking=True) ^ 0xFF       # produced on the side stream
                idx.search_device(qd.data_ptr(), nq, 100, out_i.data_ptr(), out_d.data_ptr(), stream=side.cuda_stream)
            side.synchronize()
            return out_i.cpu().numpy(), out_d.cpu().numpy()

        for order in ((130, 7), (7, 130)):                           # workspace growth both ways
            for nq in order:
                a, b = run(nq), run(nq)
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
                assert np.array_equal(a[0], host[nq][0]) and np.array_equal(a[1], host[nq][1]), nq
            idx.close()
            idx = lib.BinaryGallery.from_host(g)                     # a fresh handle: the second order grows from nothing
    finally:
        idx.close()
    ids_t, dist_t, _ = hamming_truth(g, q[:7], 100)
    assert np.array_equal(host[7][0], ids_t) and np.array_equal(host[7][1], dist_t)


@pytest.mark.parametrize("d", [8, 64, 2048])
@pytest.mark.parametrize("n", [1, 65])
def test_sign_packing(lib, d, n):
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(d + n)
    x = rng.standard_normal((n, d + 8)).astype(np.float32)            # row stride d + 8
    special = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1e-45, -1e-45, 1e-39], np.float32)
    x[:, :8] = special[np.argsort(rng.random((n, 8)), axis=1)]        # every row: the eight special values in some order
    x[-1, d - 1] = np.float32(1e-45)
    want = lib.pack_bits(x[:, :d] > 0)
    xt = torch.from_numpy(x).to(dev)
    out = torch.zeros((n, d // 8 + 3), dtype=torch.uint8, device=dev)  # output row stride d / 8 + 3
    s = torch.cuda.current_stream().cuda_stream
    lib.pack_sign_bits_device(xt.data_ptr(), n, d, out.data_ptr(), row_stride=d + 8, out_row_stride=d // 8 + 3, stream=s)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[:, :d // 8], want) and (got[:, d // 8:] == 0).all()
    idx = lib.BinaryGallery.empty(n + 70, d)
    try:
        idx.append(want[:1])                                         # the signed rows land behind a row that is there already
        idx.append_sign_device(xt.data_ptr(), n, d, row_stride=d + 8, stream=s)
        torch.cuda.synchronize()
        assert idx.n == n + 1
        assert np.array_equal(idx.get_codes(1, n), want)
        ids, dist, _ = idx.search(want[-1:], 1)
        assert dist[0, 0] == 0
    finally:
        idx.close()


def test_matching_greedyhash_hip(lib):
    from isehr_amd.nnsearch import matching_Greedyhash_hip
    z = np.load(GOLD)
    train, test, K, idx_ref = z["train"], z["test"], int(z["K"]), z["idx"]
    idx, tpq = matching_Greedyhash_hip(K, train, test)
    assert idx.dtype == np.int64 and idx.shape == (7, K) and tpq > 0
    assert np.array_equal(idx, greedyhash_restated(K, train, test))
    assert tie_aware_equal(idx_ref, idx, train, test) == []
    rng = np.random.default_rng(8)
    train = rng.integers(0, 2, size=(3000, 100), dtype=np.int64)      # code_len 100: padded to 104
    test = rng.integers(0, 2, size=(9, 100), dtype=np.int64)
    test[4] = train[2999]
    idx, _ = matching_Greedyhash_hip(50, train, test)
    assert np.array_equal(idx, greedyhash_restated(50, train, test))
    idx_b, _ = matching_Greedyhash_hip(50, train.astype(bool), test.astype(bool))
    assert np.array_equal(idx_b, idx)


def test_knn_hamming(lib):
    from isehr_amd.knn import KNN
    g, q = _codes(13, 257, 64, 3)
    knn = KNN(g, "hamming")
    try:
        dist, ids = knn.search(q, 5)
        mask = np.arange(257) % 2 == 0
        dist_m, ids_m = knn.search(q, 5, allow=mask)
    finally:
        knn.close()
    assert dist.dtype == np.int32 and ids.dtype == np.int64 and dist.shape == ids.shape == (3, 5)
    ids_t, dist_t, _ = hamming_truth(g, q, 5)
    assert np.array_equal(ids, ids_t) and np.array_equal(dist, dist_t)
    ids_t, dist_t, _ = hamming_truth(g, q, 5, allowed=mask)
    assert np.array_equal(ids_m, ids_t) and np.array_equal(dist_m, dist_t)
    assert (knn.N, knn.D) == (257, 64)
