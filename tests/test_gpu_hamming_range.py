"""GPU: radius search and self-join of the binary index (csrc/hamming_range.hip, csrc/api_hamming.hip) against the numpy truth of
tests/_hamming_range_truth.py.  The answer is integer and fully determined -- lims, ids and distances are compared with
array_equal, hits by (distance asc, id asc)."""
import ctypes as C

import numpy as np
import pytest

from _hamming_range_truth import distance_matrix, pairs_truth, range_truth
from _hamming_truth import hamming_truth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from isehr_amd import _lib
    _lib.load()
    return _lib


def _flip(rng, code, nflip):
    out = code.copy()
    for j in rng.choice(code.size * 8, size=nflip, replace=False):
        out[j >> 3] ^= np.uint8(1 << (j & 7))
    return out


def _planted(seed, n, nbits, nq, radius):
    """random codes; queries 0 .. 3 are gallery rows with 0, 1, radius and radius + 1 bits flipped: the bound from both sides"""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 256, size=(n, nbits // 8), dtype=np.uint8)
    q = rng.integers(0, 256, size=(nq, nbits // 8), dtype=np.uint8)
    for i, f in enumerate((0, 1, radius, radius + 1)):
        if i < nq and f <= nbits:
            q[i] = _flip(rng, g[(37 * i + n // 2) % n], f)
    return g, q


def _same(got, want):
    assert got[0].dtype == np.int64 and got[1].dtype == np.int64 and got[2].dtype == np.int32
    assert np.array_equal(got[0], want[0]), (got[0][:8], want[0][:8])
    assert np.array_equal(got[2], want[2])
    assert np.array_equal(got[1], want[1])


def _head(truth, nq):
    lims, ids, dist = truth
    return lims[:nq + 1], ids[:lims[nq]], dist[:lims[nq]]


MID = {8: 2, 40: 6, 64: 9, 2048: 900, 4096: 1900}       # random codes lie near nbits / 2: only the planted copies are this close


@pytest.mark.parametrize("nbits", [8, 40, 64, 2048, 4096])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4099])
def test_shape_sweep(lib, n, nbits):
    r = MID[nbits]
    g, q = _planted(nbits * 11 + n, n, nbits, 130, r)
    dmat = distance_matrix(g, q)
    assert nbits == 8 or n < 4 or (dmat[2, (37 * 2 + n // 2) % n] == r and dmat[3, (37 * 3 + n // 2) % n] == r + 1)
    idx = lib.BinaryGallery.from_host(g)
    try:
        for radius in (0, r, nbits):
            want = range_truth(g, q, radius, dmat=dmat)
            _same(idx.range_search(q, radius)[:3], want)
            if radius == nbits:                            # every row for every query, by (distance, id): far above 2048 at n = 4099
                assert np.array_equal(np.diff(want[0]), np.full(130, n))
            if radius == r:
                for nq in (1, 5):
                    _same(idx.range_search(q[:nq], radius)[:3], _head(want, nq))
    finally:
        idx.close()


def test_radius_below_every_distance(lib):
    rng = np.random.default_rng(1)
    g = rng.integers(0, 256, size=(300, 256), dtype=np.uint8)
    q = rng.integers(0, 256, size=(5, 256), dtype=np.uint8)
    dmin = int(distance_matrix(g, q).min())
    assert dmin > 800
    idx = lib.BinaryGallery.from_host(g)
    try:
        for radius in (0, dmin - 1):
            lims, ids, dist, _ = idx.range_search(q, radius)
            assert np.array_equal(lims, np.zeros(6, np.int64)) and ids.size == 0 and dist.size == 0
        lims, ids, dist, _ = idx.range_search(q, dmin)
        assert lims[-1] >= 1 and (dist == dmin).all()
    finally:
        idx.close()


@pytest.mark.parametrize("early", [0, 1])
def test_mid_radius_on_both_sides_of_the_early_exit(lib, early):
    """2048-bit random codes lie near 1024 bits apart.  Radius 900: the planted copies only, and the partial sums of most blocks
    pass it a few words before the end; radius 1040: thousands of hits per query and no block can be dropped; radius 0 and 100:
    every block but a copy's is dropped after the first words.  The option only changes the work."""
    g, q = _planted(77, 4099, 2048, 130, 900)
    dmat = distance_matrix(g, q)
    idx = lib.BinaryGallery.from_host(g)
    lib.set_global_option("hamming_range_early_exit", early)
    try:
        for radius in (0, 100, 900, 901, 1040):
            want = range_truth(g, q, radius, dmat=dmat)
            _same(idx.range_search(q, radius)[:3], want)
            if radius == 1040:
                assert np.diff(want[0]).min() > 2500
        # the self-join goes through the same loop
        lims, ids, dist, _ = idx.self_range(100, 1000, 1000)
        _same((lims, ids, dist), range_self_truth(g, 100, 1000, 1000))
    finally:
        lib.set_global_option("hamming_range_early_exit", 1)
        idx.close()


def range_self_truth(codes, row0, nrows, radius):
    """the self-join as a composition: range search with the stored rows as queries, hits j > i kept"""
    lims, ids, dist = range_truth(codes, codes[row0:row0 + nrows], radius)
    qi = np.repeat(np.arange(row0, row0 + nrows, dtype=np.int64), np.diff(lims))
    keep = ids > qi
    counts = np.bincount((qi - row0)[keep], minlength=nrows)
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), ids[keep], dist[keep]


def test_tie_classes_are_ordered_by_id(lib):
    rng = np.random.default_rng(2)
    base = rng.integers(0, 256, size=(4, 8), dtype=np.uint8)
    base[1] = _flip(rng, base[0], 3)
    base[2] = _flip(rng, base[0], 3)
    g = base[rng.integers(0, 4, size=1500)]               # four distinct codes, hundreds of rows each
    q = np.stack([base[0], base[1], _flip(rng, base[0], 1)])
    idx = lib.BinaryGallery.from_host(g)
    try:
        for radius in (0, 3, 6, 64):
            got = idx.range_search(q, radius)[:3]
            _same(got, range_truth(g, q, radius))
            for i in range(3):
                ids, dist = got[1][got[0][i]:got[0][i + 1]], got[2][got[0][i]:got[0][i + 1]]
                for d in np.unique(dist):
                    assert (np.diff(ids[dist == d]) > 0).all()
        assert idx.range_search(q, 64)[0][-1] == 3 * 1500
    finally:
        idx.close()


def test_allow_bitmap_row_offset_and_append(lib):
    import torch
    g, q = _planted(9, 1000, 64, 7, 9)
    rng = np.random.default_rng(10)
    allowed = rng.random(1000) < 0.4
    allowed[[(37 * i + 500) % 1000 for i in range(4)]] = [True, False, True, True]
    off = 10 ** 9
    dmat = distance_matrix(g, q)
    one = lib.BinaryGallery.from_host(g, row_offset=off)
    pieces = lib.BinaryGallery.empty(1100, 64, row_offset=off)
    try:
        for lo, hi in ((0, 1), (1, 64), (64, 193), (193, 1000)):
            pieces.append(g[lo:hi])
        assert pieces.n == 1000
        bits = lib.allow_bitmap(allowed, 1000)
        bits_dev = torch.from_numpy(np.asarray(bits).view(np.int64)).cuda()
        for radius in (9, 28, 64):
            want = range_truth(g, q, radius, row_offset=off, allowed=allowed, dmat=dmat)
            assert want[1].size == 0 or want[1].min() >= off
            for idx in (one, pieces):
                _same(idx.range_search(q, radius, allow=allowed)[:3], want)                      # bool mask -> host bitmap
                _same(idx.range_search(q, radius, allow=np.flatnonzero(allowed) + off)[:3], want)  # global ids
                _same(idx.range_search(q, radius, allow_ptr=bits_dev.data_ptr())[:3], want)      # device bitmap
                _same(idx.range_search(q, radius)[:3], range_truth(g, q, radius, row_offset=off, dmat=dmat))
        none = np.zeros(1000, bool)
        assert one.range_search(q, 64, allow=none)[0][-1] == 0
    finally:
        one.close()
        pieces.close()


def _device_search(lib, idx, q, radius, cap, allow_ptr=None):
    import torch
    qd = torch.from_numpy(np.ascontiguousarray(q)).cuda()
    lims = torch.full((q.shape[0] + 1,), -5, dtype=torch.int64, device="cuda")
    ids = torch.full((max(cap, 1),), -9, dtype=torch.int64, device="cuda")
    dist = torch.full((max(cap, 1),), -9, dtype=torch.int32, device="cuda")
    idx.range_search_device(qd.data_ptr(), q.shape[0], radius, cap, lims.data_ptr(), ids.data_ptr(), dist_ptr=dist.data_ptr(),
                            allow_ptr=allow_ptr, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return lims.cpu().numpy(), ids.cpu().numpy(), dist.cpu().numpy()


def test_query_chunking_does_not_change_the_answer(lib):
    """the workspace bound shrunk to its floor: chunks of 64 queries (130 -> 64, 64, 2), counted in one sweep and filled in a
    second; host form, device form and self-join"""
    g, q = _planted(21, 700, 2048, 130, 900)
    dmat = distance_matrix(g, q)
    idx = lib.BinaryGallery.from_host(g)
    try:
        for radius in (900, 1030):
            want = range_truth(g, q, radius, dmat=dmat)
            whole = idx.range_search(q, radius)[:3]
            whole_self = idx.self_range(3, 650, radius)[:3]
            lib.set_global_option("hamming_range_bytes", 1)
            try:
                chunked = idx.range_search(q, radius)[:3]
                total = int(want[0][-1])
                lims, ids, dist = _device_search(lib, idx, q, radius, total + 3)
                chunked_self = idx.self_range(3, 650, radius)[:3]
            finally:
                lib.set_global_option("hamming_range_bytes", 0)
            _same(whole, want)
            _same(chunked, want)
            _same((lims, ids[:total], dist[:total]), want)
            assert (ids[total:] == -9).all()
            _same(whole_self, range_self_truth(g, 3, 650, radius))
            _same(chunked_self, whole_self)
        assert lib.get_global_option("hamming_range_bytes") == 1 << 30
    finally:
        idx.close()


def test_capacity_protocol(lib):
    g, q = _planted(31, 500, 64, 40, 9)
    want = range_truth(g, q, 26)
    total = int(want[0][-1])
    assert total > 100
    L = lib.load()
    idx = lib.BinaryGallery.from_host(g)
    P = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    try:
        for cap, rc_want in ((total - 1, lib.MI_ERR_CAPACITY), (0, lib.MI_ERR_CAPACITY), (total, 0)):
            lims = np.full(41, -5, np.int64)
            ids = np.full(total + 4, -9, np.int64)
            dist = np.full(total + 4, -9, np.int32)
            rc = L.mi_hamming_range_search(idx._h, P(q), 40, 8, 26, None, 0, cap, P(lims), P(ids) if cap else None, P(dist), None)
            assert rc == rc_want, (cap, rc, L.mi_last_error())
            assert np.array_equal(lims, want[0])                         # always complete
            if rc:
                assert b"max_results" in L.mi_last_error()
                assert (ids == -9).all() and (dist == -9).all()          # nothing written
            else:
                assert np.array_equal(ids[:total], want[1]) and np.array_equal(dist[:total], want[2])
                assert (ids[total:] == -9).all() and (dist[total:] == -9).all()
            # the device form decides on the device and returns MI_OK either way
            lims, ids, dist = _device_search(lib, idx, q, 26, cap)
            assert np.array_equal(lims, want[0])
            if cap < total:
                assert (ids == -9).all() and (dist == -9).all()
            else:
                assert np.array_equal(ids[:total], want[1]) and np.array_equal(dist[:total], want[2])
        # out_dist may be NULL
        lims = np.zeros(41, np.int64)
        ids = np.zeros(total, np.int64)
        assert L.mi_hamming_range_search(idx._h, P(q), 40, 8, 26, None, 0, total, P(lims), P(ids), None, None) == 0
        assert np.array_equal(ids, want[1])
        # self-join: the same protocol
        sw = range_self_truth(g, 10, 300, 26)
        st = int(sw[0][-1])
        assert st > 10
        lims = np.full(301, -5, np.int64)
        ids = np.full(st, -9, np.int64)
        assert L.mi_hamming_self_range(idx._h, 10, 300, 26, st - 1, P(lims), P(ids), None, None) == lib.MI_ERR_CAPACITY
        assert np.array_equal(lims, sw[0]) and (ids == -9).all()
        assert L.mi_hamming_self_range(idx._h, 10, 300, 26, st, P(lims), P(ids), None, None) == 0
        assert np.array_equal(ids, sw[1])
        for row0, nrows in ((501, 0), (0, 501), (400, 101)):
            assert L.mi_hamming_self_range(idx._h, row0, nrows, 1, st, P(lims), P(ids), None, None) == lib.MI_ERR_INVALID
        assert L.mi_hamming_self_range(idx._h, 500, 0, 1, st, P(lims), P(ids), None, None) == 0 and lims[0] == 0
        # the Python wrapper retries once with the exact size
        _same(idx.range_search(q, 26, max_results=1)[:3], want)
        _same(idx.self_range(10, 300, 26, max_results=0)[:3], sw)
    finally:
        idx.close()


def test_consistent_with_top_k(lib):
    g, q = _planted(41, 3000, 256, 9, 40)
    k = 50
    ids_t, dist_t, _ = hamming_truth(g, q, k)
    idx = lib.BinaryGallery.from_host(g)
    try:
        top_ids, top_dist, _ = idx.search(q, k)
        assert np.array_equal(top_ids, ids_t) and np.array_equal(top_dist, dist_t)
        for i in range(9):
            lims, ids, dist, _ = idx.range_search(q[i:i + 1], int(top_dist[i, k - 1]))
            assert lims[1] >= k
            assert np.array_equal(ids[:k], top_ids[i]) and np.array_equal(dist[:k], top_dist[i])
    finally:
        idx.close()


def test_device_form_and_lsh_index(lib):
    import torch
    rng = np.random.default_rng(51)
    x = rng.standard_normal((900, 48)).astype(np.float32)
    xq = x[:20] + 0.05 * rng.standard_normal((20, 48)).astype(np.float32)
    lsh = lib.LSHIndex.from_host(x, nbits=128)
    try:
        qcodes = lsh.encode(xq)
        g = lsh.get_codes()
        allowed = rng.random(900) < 0.5
        for radius, allow in ((10, None), (40, None), (40, allowed), (128, None)):
            want = range_truth(g, qcodes, radius, allowed=allow)
            host = lsh.gallery.range_search(qcodes, radius, allow=allow)[:3]
            _same(host, want)
            _same(lsh.range_search(xq, radius, allow=allow)[:3], host)
            _same(lsh.range_search(xq, radius, allow=allow, max_results=1)[:3], host)     # the retry on the device form
            total = int(want[0][-1])
            bits_dev = None if allow is None else torch.from_numpy(np.asarray(lib.allow_bitmap(allow, 900)).view(np.int64)).cuda()
            lims, ids, dist = _device_search(lib, lsh.gallery, qcodes, radius, total,
                                             allow_ptr=None if allow is None else bits_dev.data_ptr())
            _same((lims, ids[:total], dist[:total]), host)
        assert want[0][-1] == 20 * 900
        from isehr_amd.dedup import near_duplicate_pairs_hamming
        _same3 = [np.array_equal(a, b) for a, b in zip(near_duplicate_pairs_hamming(lsh, 30, batch=200), pairs_truth(g, 30))]
        assert _same3 == [True] * 3
    finally:
        lsh.gallery.close()


@pytest.mark.parametrize("n", [1, 65, 300, 2500])
def test_self_join(lib, n):
    from isehr_amd.dedup import near_duplicate_pairs_hamming
    rng = np.random.default_rng(60 + n)
    g = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    for grp in range(n // 12):                             # duplicate groups: exact copies and copies 1 .. 4 bits away
        src = int(rng.integers(0, n))
        for dst in rng.integers(0, n, size=int(rng.integers(1, 6))):
            g[dst] = _flip(rng, g[src], int(rng.integers(0, 5)))
    idx = lib.BinaryGallery.from_host(g)
    try:
        for radius in (0, 3, 8) + ((256,) if n <= 300 else ()):
            want = pairs_truth(g, radius)
            if n >= 65 and radius:
                assert want[0].size > n // 12 and {0, 1, 2, 3} <= set(want[2].tolist())
            for batch in (1, 64, 100, n + 5) if n <= 300 else (64, 100, n):
                got = near_duplicate_pairs_hamming(idx, radius, batch=batch)
                assert [a.dtype for a in got] == [np.int64, np.int64, np.int32]
                assert all(np.array_equal(a, b) for a, b in zip(got, want)), (radius, batch)
            # the composition, from a row that is no multiple of 64 and over a range that ends inside a block
            row0, nrows = min(n - 1, 37), max(1, (n - min(n - 1, 37)) * 2 // 3)
            _same(idx.self_range(row0, nrows, radius)[:3], range_self_truth(g, row0, nrows, radius))
        if n == 300:
            assert pairs_truth(g, 256)[0].size == 300 * 299 // 2
            _same(idx.self_range(299, 1, 256)[:3], (np.zeros(2, np.int64), np.empty(0, np.int64), np.empty(0, np.int32)))
            _same(idx.self_range(63, 1, 256)[:3], range_self_truth(g, 63, 1, 256))
    finally:
        idx.close()
