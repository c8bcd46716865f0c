"""GPU: the IVF index over PQ codes (csrc/ivfpq.hip, csrc/api_ivfpq.hip) against a pure-numpy truth (tests/_ivfpq_truth.py).
The contract is bit-exact: ids are compared with ==, distances on their bits (view(uint32)), probes with ==."""
import ctypes as C

import numpy as np
import pytest

from _ivfpq_truth import ivfpq_truth, probe_truth
from _pq_truth import encode_truth, pq_truth
from test_gpu_pq import SHAPES

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


def _problem(seed, n, nlist, M, Ks, L, nq, lists=None):
    """seeded centroids, codebooks, codes, lists and queries.  Row n - 1 is a copy of row 0 in ANOTHER list and row n // 3 a copy
    of row n // 2 in the SAME list (exact distance ties across and inside lists); query 0 is the reconstruction of row n // 2
    (distance 0 in every book)"""
    rng = np.random.default_rng(seed)
    Cb = rng.standard_normal((M, Ks, L)).astype(np.float32)
    G = rng.standard_normal((nlist, M * L)).astype(np.float32)
    codes = rng.integers(0, Ks, size=(n, M), dtype=np.uint8)
    given = lists is not None
    lists = np.asarray(lists, np.uint8) if given else rng.integers(0, nlist, size=n).astype(np.uint8)
    if n > 4:
        codes[n - 1], codes[n // 3] = codes[0], codes[n // 2]
        if not given:
            lists[n - 1], lists[n // 3] = (int(lists[0]) + 1) % nlist, lists[n // 2]
    q = rng.standard_normal((nq, M * L)).astype(np.float32)
    q[0] = np.concatenate([Cb[m, codes[n // 2, m]] for m in range(M)])
    return G, Cb, codes, lists, q


# (N, nlist, nprobe, shape, k, nq): every N {1, 63, 64, 65, 257, 5000, 70001}, nlist {2, 7, 256}, nprobe {1, 3, nlist}, every
# (M, Ks, L) of test_gpu_pq.SHAPES, k {1, 100, 2048}, nq {1, 5, 130}.  nlist = 256 beside a small N leaves most lists empty;
# 70001 rows in 2 lists span 9 slabs of 4096 candidates per list, and k = 2048 makes the merge fold more than 2048 keys
SWEEP = [
    (1, 2, 1, 0, 1, 1), (1, 7, 7, 1, 100, 5), (63, 7, 3, 2, 100, 130), (63, 256, 256, 4, 2048, 1),
    (64, 2, 2, 1, 1, 5), (64, 256, 3, 3, 100, 5), (65, 7, 1, 5, 100, 1), (65, 2, 1, 2, 2048, 130),
    (257, 7, 3, 4, 2048, 5), (257, 256, 1, 0, 1, 130), (257, 2, 2, 3, 100, 1),
    (5000, 7, 7, 2, 2048, 5), (5000, 256, 3, 1, 100, 130), (5000, 2, 1, 5, 1, 5), (5000, 7, 1, 4, 100, 1),
    (70001, 2, 2, 2, 2048, 5), (70001, 2, 1, 1, 100, 130), (70001, 7, 3, 0, 2048, 1), (70001, 256, 256, 4, 100, 5),
    (70001, 256, 3, 3, 1, 1),
]


@pytest.mark.parametrize("n,nlist,nprobe,shape,k,nq", SWEEP)
def test_search_is_the_truth(lib, n, nlist, nprobe, shape, k, nq):
    M, Ks, L = SHAPES[shape]
    G, Cb, codes, lists, q = _problem(n * 31 + nlist * 7 + nprobe + shape + k + nq, n, nlist, M, Ks, L, nq)
    off = 1000 * (n % 2)
    probes = probe_truth(q, G, nprobe)
    want = ivfpq_truth(q, Cb, codes, lists, probes, k, row_offset=off)
    with lib.IVFPQIndex.from_codes(G, Cb, codes, lists, row_offset=off) as idx:
        assert (idx.n, idx.m, idx.ks, idx.d, idx.nlist, idx.row_offset, idx.capacity) == (n, M, Ks, M * L, nlist, off, n)
        assert np.array_equal(idx.list_sizes(), np.bincount(lists, minlength=nlist))
        assert np.array_equal(idx.probe(q, nprobe), probes)
        ids, dist, _ = idx.search(q, k, nprobe=nprobe)
        assert idx.hbm_bytes > 0
    assert ids.dtype == np.int64 and dist.dtype == np.float32 and ids.shape == (nq, k)
    assert np.array_equal(_bits(dist), _bits(want[1]))
    assert np.array_equal(ids, want[0])
    if nprobe == nlist:
        assert _same((ids, dist), pq_truth(q, Cb, codes, k, row_offset=off))
    found = (want[0] >= 0).sum(1)
    assert (ids[np.arange(k)[None, :] >= found[:, None]] == -1).all()


def test_probes_and_first_probe(lib):
    rng = np.random.default_rng(5)
    for nlist, (M, Ks, L) in ((2, SHAPES[0]), (7, SHAPES[1]), (256, SHAPES[3]), (256, SHAPES[5])):
        d = M * L
        G = rng.standard_normal((nlist, d)).astype(np.float32)
        G[nlist - 1] = G[0]                                             # two identical centroids: the lower id comes first
        Cb = rng.standard_normal((M, Ks, L)).astype(np.float32)
        q64 = rng.standard_normal((130, d))
        q64[3] = G[0].astype(np.float64) + 2.0 ** -30                   # below float32 resolution
        q64[4] = G[0]
        q32 = q64.astype(np.float32)
        with lib.IVFPQIndex.empty(G, Cb, 200) as idx:
            full32, full64 = probe_truth(q32, G, nlist), probe_truth(q64, G, nlist)       # the first nprobe columns are the truth
            for nprobe in sorted({1, min(3, nlist), nlist}):
                for name, q, full in (("f32", q32, full32), ("f64", q64, full64), ("transposed view", np.asfortranarray(q32), full32),
                                      ("one", q32[:1], full32[:1]), ("five", q64[:5], full64[:5])):
                    got = idx.probe(q, nprobe)
                    assert got.dtype == np.int32 and np.array_equal(got, full[:, :nprobe]), (nlist, nprobe, name)
            full = idx.probe(q32[4:5], nlist)[0]
            assert full[0] == 0 and full[1] == nlist - 1
            # a float32 gallery row used as a query: its first probe is its own list
            idx.add(q32)
            _, lists = idx.get_rows()
            assert np.array_equal(idx.probe(q32, 1)[:, 0], lists)
            assert np.array_equal(lists, encode_truth(q32, G[None])[:, 0])
            with pytest.raises(RuntimeError, match="finite"):
                idx.probe(np.full((1, d), np.nan, np.float32), 1)
            with pytest.raises(RuntimeError, match="finite"):
                idx.search(np.full((1, d), np.inf, np.float32), 1)


def test_special_lists_and_padding(lib):
    """empty lists, one list holding every row, lists of exactly 64 and 65 rows, fewer than k candidates"""
    M, Ks, L = SHAPES[2]
    sizes = [64, 65, 0, 128, 0, 1, 0]                                    # 258 rows in 7 lists
    lists = np.random.default_rng(1).permutation(np.repeat(np.arange(7), sizes))
    G, Cb, codes, lists, q = _problem(21, 258, 7, M, Ks, L, 5, lists=lists)
    every = np.tile(np.arange(7), (5, 1))
    with lib.IVFPQIndex.from_codes(G, Cb, codes, lists, row_offset=5) as idx:
        assert idx.list_sizes().tolist() == sizes
        for lst in range(7):                                            # one list at a time: 64, 65, none, ...
            pr = np.full((5, 1), lst)
            got = idx.search(q, 100, probes=pr)[:2]
            assert _same(got, ivfpq_truth(q, Cb, codes, lists, pr, 100, row_offset=5)), lst
            assert ((got[0] >= 0).sum(1) == min(sizes[lst], 100)).all()
        for k in (1, 100, 2048):
            assert _same(idx.search(q, k, probes=every)[:2], pq_truth(q, Cb, codes, k, row_offset=5)), k
        for nprobe in (1, 3, 7):
            pr = probe_truth(q, G, nprobe)
            assert _same(idx.search(q, 300, nprobe=nprobe)[:2], ivfpq_truth(q, Cb, codes, lists, pr, 300, row_offset=5)), nprobe
    G, Cb, codes, _, q = _problem(22, 5000, 7, M, Ks, L, 5)
    one = np.full(5000, 4, np.uint8)
    with lib.IVFPQIndex.from_codes(G, Cb, codes, one) as idx:
        assert idx.list_sizes().tolist() == [0, 0, 0, 0, 5000, 0, 0]
        assert _same(idx.search(q, 100, nprobe=7)[:2], pq_truth(q, Cb, codes, 100))
        pr = probe_truth(q, G, 1)
        got = idx.search(q, 100, nprobe=1)
        assert _same(got[:2], ivfpq_truth(q, Cb, codes, one, pr, 100))
        assert ((got[0] == -1).all(1) == (pr[:, 0] != 4)).all()


def test_every_list_probed_is_the_pq_index(lib):
    for (n, nlist, k, nq), shape in zip([(5000, 7, 100, 130), (70001, 2, 2048, 5), (257, 256, 2048, 5), (65, 7, 1, 1)], (3, 2, 4, 5)):
        M, Ks, L = SHAPES[shape]
        G, Cb, codes, lists, q = _problem(n + nlist, n, nlist, M, Ks, L, nq)
        with lib.PQIndex.from_codes(Cb, codes, row_offset=9) as flat, lib.IVFPQIndex.from_codes(G, Cb, codes, lists, row_offset=9) as idx:
            want = flat.search(q, k)[:2]
            assert _same(idx.search(q, k, nprobe=nlist)[:2], want), (n, nlist)
        assert _same(want, pq_truth(q, Cb, codes, k, row_offset=9))


def test_allow_bitmap(lib):
    import torch
    n, k = 5000, 100
    M, Ks, L = SHAPES[1]
    G, Cb, codes, lists, q = _problem(30, n, 7, M, Ks, L, 5)
    rng = np.random.default_rng(3)
    probes = probe_truth(q, G, 3)
    masks = {"random": rng.random(n) < 0.3, "few": np.isin(np.arange(n), [0, 63, 64, 4999, n // 2, n // 3]), "none": np.zeros(n, bool),
             "all": np.ones(n, bool), "a probed list cleared": lists != probes[0, 0],
             "every probed list of query 0 cleared": ~np.isin(lists, probes[0])}
    with lib.IVFPQIndex.from_codes(G, Cb, codes, lists, row_offset=7000) as idx:
        plain = idx.search(q, k, nprobe=3)[:2]
        for name, allow in masks.items():
            want = ivfpq_truth(q, Cb, codes, lists, probes, k, row_offset=7000, allowed=allow)
            got = idx.search(q, k, nprobe=3, allow=allow)[:2]
            assert _same(got, want), name
            bits = lib.allow_bitmap(allow, n, 7000)
            dbits = torch.from_numpy(np.ascontiguousarray(bits).view(np.int64).copy()).to("cuda:0")
            torch.cuda.synchronize()
            assert _same(idx.search(q, k, nprobe=3, allow_ptr=dbits.data_ptr())[:2], want), name + " (device bitmap)"
            if name == "all":
                assert _same(got, plain)
        assert (idx.search(q, k, nprobe=3, allow=masks["every probed list of query 0 cleared"])[0][0] == -1).all()


def _device_search(torch, idx, q, k, nprobe, probes=None, stream=None):
    dev = torch.device("cuda", 0)
    nq = q.shape[0]
    out_i = torch.empty((nq, k), dtype=torch.int64, device=dev)
    out_d = torch.empty((nq, k), dtype=torch.float32, device=dev)
    qd = torch.from_numpy(np.ascontiguousarray(q, np.float32)).to(dev)
    pd = None if probes is None else torch.from_numpy(np.ascontiguousarray(probes, np.int32)).to(dev)
    torch.cuda.synchronize()
    idx.search_device(qd.data_ptr(), nq, k, out_i.data_ptr(), out_d.data_ptr(), nprobe=nprobe,
                      probes_ptr=None if pd is None else pd.data_ptr(), stream=None if stream is None else stream.cuda_stream)
    (torch.cuda.current_stream() if stream is None else stream).synchronize()
    torch.cuda.synchronize()
    return out_i.cpu().numpy(), out_d.cpu().numpy()


def test_explicit_probes(lib):
    import torch
    M, Ks, L = SHAPES[2]
    G, Cb, codes, lists, q = _problem(40, 5000, 7, M, Ks, L, 5)
    pr = np.array([[0, 1, 2, 3], [6, -1, 6, 6], [-1, -1, -1, -1], [5, 4, 5, -1], [2, 2, 1, 1]], np.int32)
    with lib.IVFPQIndex.from_codes(G, Cb, codes, lists, row_offset=3) as idx:
        want = ivfpq_truth(q, Cb, codes, lists, pr, 100, row_offset=3)
        host = idx.search(q, 100, probes=pr)[:2]
        assert _same(host, want)
        assert (host[0][2] == -1).all() and np.isposinf(host[1][2]).all()
        assert _same(idx.search(q, 100, probes=pr.astype(np.int64))[:2], want)
        assert _same(_device_search(torch, idx, q, 100, 4, pr), want)
        # on the device an entry out of range acts as -1
        wild = pr.copy()
        wild[1, 1], wild[2, 0], wild[2, 3], wild[3, 3] = 7, 2 ** 31 - 1, -2 ** 31, -5
        assert _same(_device_search(torch, idx, q, 100, 4, wild), want)
        # on the host it is an error: with the wrapper's own check out of the way, the library's answers
        bad = pr.copy()
        bad[4, 0] = 7
        with pytest.raises(ValueError, match="nlist = 7"):
            idx.search(q, 100, probes=bad)
        out = np.zeros((5, 100), np.int64)
        P = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
        rc = lib.load().mi_ivfpq_search(idx._h, P(q), 5, lib.MI_F32, q.shape[1], 1, 100, 4, P(bad), None, lib.MI_HOST, P(out), None, None)
        assert rc == lib.MI_ERR_INVALID and b"probe entry" in lib.load().mi_last_error()
        rc = lib.load().mi_ivfpq_search(idx._h, P(q), 5, lib.MI_F32, q.shape[1], 1, 100, 8, None, None, lib.MI_HOST, P(out), None, None)
        assert rc == lib.MI_ERR_INVALID and b"nprobe must" in lib.load().mi_last_error()
        assert lib.load().mi_ivfpq_search(idx._h, P(q), 0, lib.MI_F32, q.shape[1], 1, 100, 4, None, None, lib.MI_HOST, None, None, None) == 0


def test_append_in_any_order_answers_identically(lib):
    import torch
    M, Ks, L = SHAPES[1]
    rng = np.random.default_rng(50)
    n, nlist = 3000, 7
    G = rng.standard_normal((nlist, M * L)).astype(np.float32)
    Cb = rng.standard_normal((M, Ks, L)).astype(np.float32)
    x = rng.standard_normal((n, M * L)).astype(np.float32)
    x[n - 1], x[n // 3] = x[0], x[n // 2]
    codes, lists = encode_truth(x, Cb), encode_truth(x, G[None])[:, 0]
    q = rng.standard_normal((5, M * L)).astype(np.float32)
    pr = probe_truth(q, G, 3)
    want = ivfpq_truth(q, Cb, codes, lists, pr, 2048)
    cuts = [0, 1, 700, 764, 2999, 3000]                                  # five steps; the blocks of the lists interleave
    once = lib.IVFPQIndex.from_codes(G, Cb, codes, lists)
    steps = lib.IVFPQIndex.empty(G, Cb, 3100)
    raw = lib.IVFPQIndex.empty(G, Cb, 3000)
    try:
        for a, b in zip(cuts[:-1], cuts[1:]):
            steps.append_codes(codes[a:b], lists[a:b])
            raw.add(x[a:b] if a % 2 else x[a:b].astype(np.float64))
        for name, idx in (("create", once), ("append_codes", steps), ("add", raw)):
            assert idx.n == n, name
            assert _same(idx.search(q, 2048, nprobe=3)[:2], want), name
            assert _same(idx.search(q, 100, nprobe=nlist)[:2], pq_truth(q, Cb, codes, 100)), name
            got_codes, got_lists = idx.get_rows()
            assert np.array_equal(got_codes, codes) and np.array_equal(got_lists, lists), name
            got_codes, got_lists = idx.get_rows(699, 70)
            assert np.array_equal(got_codes, codes[699:769]) and np.array_equal(got_lists, lists[699:769]), name
            assert np.array_equal(idx.list_sizes(), np.bincount(lists, minlength=nlist)), name

        # refused appends leave the index as it was: capacity, a bad byte, a bad list id; host and device data
        def state(idx):
            info = (idx._info(), idx.n, idx.capacity)
            return info, idx.list_sizes().tolist(), idx.search(q, 100, nprobe=3)[:2]

        before = state(steps)
        call = lib.load().mi_ivfpq_append_codes
        P = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
        bad_codes, bad_lists = codes[:50].copy(), lists[:50].copy()
        bad_codes[49, 2], bad_lists[49] = Ks, nlist
        with pytest.raises(RuntimeError, match="capacity"):
            steps.append_codes(codes[:101], lists[:101])
        assert call(steps._h, P(bad_codes), P(lists[:50].copy()), 50, M, lib.MI_HOST) == lib.MI_ERR_INVALID
        assert b">= ks" in lib.load().mi_last_error()
        assert call(steps._h, P(codes[:50].copy()), P(bad_lists), 50, M, lib.MI_HOST) == lib.MI_ERR_INVALID
        assert b">= nlist" in lib.load().mi_last_error()
        dev = {k: torch.from_numpy(v.copy()).to("cuda:0") for k, v in
               (("codes", codes[:50]), ("lists", lists[:50]), ("bad_codes", bad_codes), ("bad_lists", bad_lists), ("many", codes[:101]),
                ("many_lists", lists[:101]))}
        torch.cuda.synchronize()
        with pytest.raises(RuntimeError, match=">= ks"):
            steps.append_codes_device(dev["bad_codes"].data_ptr(), dev["lists"].data_ptr(), 50)
        with pytest.raises(RuntimeError, match=">= nlist"):
            steps.append_codes_device(dev["codes"].data_ptr(), dev["bad_lists"].data_ptr(), 50)
        with pytest.raises(RuntimeError, match="capacity"):
            steps.append_codes_device(dev["many"].data_ptr(), dev["many_lists"].data_ptr(), 101)
        with pytest.raises(RuntimeError, match=">= nlist"):
            lib.IVFPQIndex.from_device_ptr(G, Cb, dev["codes"].data_ptr(), dev["bad_lists"].data_ptr(), 50)
        after = state(steps)
        assert after[0] == before[0] and after[1] == before[1] and _same(after[2], before[2])
        # and device data that passes is ingested like host data
        steps.append_codes_device(dev["codes"].data_ptr(), dev["lists"].data_ptr(), 50)
        both_codes, both_lists = np.concatenate([codes, codes[:50]]), np.concatenate([lists, lists[:50]])
        assert _same(steps.search(q, 2048, nprobe=3)[:2], ivfpq_truth(q, Cb, both_codes, both_lists, pr, 2048))
        with lib.IVFPQIndex.from_device_ptr(G, Cb, dev["many"].data_ptr(), dev["many_lists"].data_ptr(), 101) as d:
            assert _same(d.search(q, 100, nprobe=3)[:2], ivfpq_truth(q, Cb, codes[:101], lists[:101], pr, 100))
    finally:
        for idx in (once, steps, raw):
            idx.close()


def test_device_path_on_a_side_stream(lib):
    import torch
    M, Ks, L = SHAPES[4]
    G, Cb, codes, lists, q = _problem(60, 5000, 7, M, Ks, L, 130)
    side = torch.cuda.Stream(device=torch.device("cuda", 0))
    with lib.IVFPQIndex.from_codes(G, Cb, codes, lists) as idx:
        host = idx.search(q, 100, nprobe=3)[:2]
        assert _same(host, ivfpq_truth(q, Cb, codes, lists, probe_truth(q, G, 3), 100))
        first = _device_search(torch, idx, q, 100, 3, stream=side)
        second = _device_search(torch, idx, q, 100, 3, stream=side)
        assert _same(first, host)
        assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()
        assert _same(_device_search(torch, idx, q[:7], 100, 3, stream=side), (host[0][:7], host[1][:7]))


def test_chunking_changes_nothing(lib):
    M, Ks, L = SHAPES[2]
    G, Cb, codes, lists, q = _problem(70, 5000, 7, M, Ks, L, 130)
    with lib.IVFPQIndex.from_codes(G, Cb, codes, lists) as idx:
        got0 = idx.search(q, 100, nprobe=3)[:2]
        try:
            lib.set_global_option("pq_matrix_bytes", 50 * 2 * 100 * 8)     # a few tens of queries per chunk
            got1 = idx.search(q, 100, nprobe=3)[:2]
            lib.set_global_option("pq_matrix_bytes", 1)                    # below one query: one query per chunk
            got2 = idx.search(q[:9], 100, nprobe=3)[:2]
        finally:
            lib.set_global_option("pq_matrix_bytes", 0)
        assert lib.get_global_option("pq_matrix_bytes") == 2 << 30
    assert _same(got0, ivfpq_truth(q, Cb, codes, lists, probe_truth(q, G, 3), 100))
    assert _same(got1, got0)
    assert _same(got2, (got0[0][:9], got0[1][:9]))


def test_infinity_and_zero_are_ordinary_values(lib):
    M, Ks, L = SHAPES[1]
    G, Cb, codes, lists, q = _problem(80, 5000, 7, M, Ks, L, 5)
    Cb[0, 1:] += np.float32(3e19)                                        # (3e19)^2 is beyond float32: entries of book 0 are +inf
    codes[:, 0] = np.where(np.arange(5000) % 3 == 0, 0, codes[:, 0])     # but codeword 0 of book 0 stays finite
    codes[2500, 0] = 0
    q[0] = np.concatenate([Cb[m, codes[2500, m]] for m in range(M)])
    pr = np.tile(np.arange(7), (5, 1))
    want = ivfpq_truth(q, Cb, codes, lists, pr, 2048)
    assert np.isposinf(want[1]).any() and (want[0][np.isposinf(want[1])] >= 0).all()      # +inf distances of real rows
    assert want[1][0, 0] == 0 and want[0][0, 0] in (codes == codes[2500]).all(1).nonzero()[0]
    with lib.IVFPQIndex.from_codes(G, Cb, codes, lists) as idx:
        assert _same(idx.search(q, 2048, nprobe=7)[:2], want)
        pr3 = probe_truth(q, G, 3)
        assert _same(idx.search(q, 2048, nprobe=3)[:2], ivfpq_truth(q, Cb, codes, lists, pr3, 2048))


def test_fit_and_the_reference_wrapper(lib):
    from isehr_amd.nnsearch import matching_PQ_Net_bucket_hip
    rng = np.random.default_rng(90)
    M, Ks, L, nlist = 4, 16, 4, 5
    centres = rng.standard_normal((nlist, M * L)) * 4
    x = (centres[rng.integers(0, nlist, size=2000)] + rng.standard_normal((2000, M * L))).astype(np.float32)
    q = (centres[rng.integers(0, nlist, size=9)] + rng.standard_normal((9, M * L))).astype(np.float32)
    with lib.IVFPQIndex.fit(x, nlist, M, Ks, iters=5, seed=42) as idx:
        G = lib.pq_train(x, 1, nlist, iters=5, seed=42)[0][0]
        Cb = lib.pq_train(x, M, Ks, iters=5, seed=42)[0]
        codes, lists = idx.get_rows()
        assert np.array_equal(lists, encode_truth(x, G[None])[:, 0]) and np.array_equal(codes, encode_truth(x, Cb))
        assert np.array_equal(idx.probe(q, 2), probe_truth(q, G, 2))
        for nprobe in (1, 2, nlist):
            assert _same(idx.search(q, 50, nprobe=nprobe)[:2], ivfpq_truth(q, Cb, codes, lists, probe_truth(q, G, nprobe), 50)), nprobe
    # the wrapper: codewords in the reference's [Ks, M * L] form, buckets from pq_train(gallery, 1, n_clusters, seed=0)
    cw = np.ascontiguousarray(Cb.transpose(1, 0, 2).reshape(Ks, M * L))
    G10 = lib.pq_train(x, 1, 10, seed=0)[0][0]
    labels = encode_truth(x, G10[None])[:, 0]
    for nprobe in (1, 3):
        got, per_query = matching_PQ_Net_bucket_hip(20, cw, q, M, codes, x, nprobe=nprobe)
        assert got.dtype == np.int64 and got.shape == (9, 20) and per_query >= 0
        pr = probe_truth(q, G10, nprobe)
        assert np.array_equal(got, ivfpq_truth(q, Cb, codes, labels, pr, 20)[0])
        assert all(np.isin(labels[got[i][got[i] >= 0]], pr[i]).all() for i in range(9))
