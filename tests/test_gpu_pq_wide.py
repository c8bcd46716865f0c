"""GPU: the wide PQ index (csrc/pq_wide.hip, csrc/api_pq_wide.hip, mi_pqw_train) against the numpy truth (tests/_pq_truth.py,
tests/_pq_wide_truth.py) and against the byte index.  The contract is bit-exact: ids and codes are compared with ==, distances,
table entries and codebooks on their float32 bits (view(uint32)).  No tolerance anywhere."""
import functools
import os

import numpy as np
import pytest

from _pq_truth import dtable64, pq_truth
from _pq_train_truth import clustered, rows_init
from _pq_wide_truth import encode_truth16, train_truth16

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


@functools.lru_cache(maxsize=None)
def _problem(n, M, Ks, L, nq):
    """seeded codebooks, codes and queries, shared and read-only; query 0 is the reconstruction of a gallery row, and a few
    gallery rows are copies of others, so that exact ties occur"""
    rng = np.random.default_rng(n + 3 * M + 5 * Ks + 7 * L)
    C = rng.standard_normal((M, Ks, L)).astype(np.float32)
    codes = rng.integers(0, Ks, size=(n, M)).astype(np.uint16)
    codes[:, 0][: min(n, Ks)] = np.arange(min(n, Ks))[::-1]              # the highest codeword of book 0 is in use
    if n > 4:
        codes[n - 1], codes[n // 3] = codes[0], codes[n // 2]
    q = rng.standard_normal((nq, M * L)).astype(np.float32)
    q[0] = np.concatenate([C[m, codes[n // 2, m]] for m in range(M)])
    for a in (C, codes, q):
        a.setflags(write=False)
    return C, codes, q


# (N, M, Ks, L, nq, K).  QT, the queries of a workgroup, is 4 for Ks <= 4096 and 2 above (1 for a single query); a group is GP book
# pairs.  N: 1, 63, 64, 65, 257, 5000 and one over a scan slab; M: 1, 3, 5 (a half-empty last dword), 16, 64; every Ks of
# {2, 256, 257, 300, 4096, 8192}; nq: 1, QT, QT + 1, 130; K: 1, 100, N, 2048.
SWEEP = [
    (1, 1, 2, 1, 1, 1),
    (63, 3, 256, 2, 4, 63),                  # nq = QT = 4, K = N
    (64, 5, 8192, 1, 1, 64),                 # QT = 1, GP = 2: groups of 2 pairs and 1 pair (ragged), the last dword half empty
    (65, 16, 8192, 1, 3, 65),                # QT = 2, nq = QT + 1, GP = 1: eight groups
    (257, 64, 257, 1, 5, 100),               # many books, small groups: GP = 15 -> 15 + 15 + 2 pairs; Ks odd: the dword table load
    (5000, 16, 300, 2, 130, 2048),           # the tables fit: one pass
    (5000, 16, 8192, 1, 1, 100),             # QT = 1, GP = 2: four full groups
    (5000, 16, 8192, 1, 2, 1),               # nq = QT = 2
    (257, 1, 4096, 8, 2, 257),
    ("slab", 3, 4096, 1, 130, 100),          # one row over a slab: a second slab of one block; GP = 1, two groups
]


@pytest.mark.parametrize("N,M,Ks,L,nq,K", SWEEP)
def test_search_is_the_truth_bit_for_bit(lib, N, M, Ks, L, nq, K):
    if N == "slab":
        N = lib.PQW_SLAB_ROWS + 1
    C, codes, q = _problem(N, M, Ks, L, nq)
    want = pq_truth(q, C, codes, K)
    with lib.WidePQIndex.from_codes(C, codes) as g:
        assert (g.n, g.d, g.m, g.ks) == (N, M * L, M, Ks)
        got = g.search(q, K)
        assert _same(got, want)
        if N == 5000 and nq == 130:
            assert np.array_equal(_bits(g.dtable(q[:5])), _bits(dtable64(q[:5], C)[1]))
            assert np.array_equal(g.get_codes(), codes) and g.get_codes().dtype == np.uint16
            assert np.array_equal(g.get_codes(4990, 7), codes[4990:4997])
            want_rows = np.concatenate([C[j][codes[:, j]] for j in range(M)], axis=1)
            assert np.array_equal(_bits(g.decode()), _bits(want_rows))
            assert _same(g.search(q.astype(np.float64), K), want)          # float64 queries that are float32 values


@pytest.mark.parametrize("Ks", [2, 255, 256])
def test_byte_range_equals_the_byte_index(lib, Ks):
    n, M, L, nq, K = 1000, 5, 3, 9, 100
    C, codes, q = _problem(n, M, Ks, L, nq)
    allow = np.random.default_rng(Ks).random(n) < 0.3
    few = np.zeros(n, bool)
    few[[3, 500, 999]] = True
    with lib.PQIndex.from_codes(C, codes.astype(np.uint8), row_offset=70) as b, lib.WidePQIndex.from_codes(C, codes, row_offset=70) as w:
        for kw in ({}, {"allow": allow}, {"allow": few}, {"allow": np.zeros(n, bool)}):
            got, want = w.search(q, K, **kw), b.search(q, K, **kw)
            assert _same(got, want), kw
        assert (got[0] == -1).all() and np.isinf(got[1]).all()
        x = np.random.default_rng(1).standard_normal((300, M * L)).astype(np.float32)
        assert np.array_equal(w.encode(x), b.encode(x))
        assert np.array_equal(_bits(w.dtable(q)), _bits(b.dtable(q)))
        assert np.array_equal(_bits(w.decode()), _bits(b.decode()))


@pytest.mark.parametrize("cls,dtype,Ks", [("PQIndex", np.uint8, 5), ("WidePQIndex", np.uint16, 300)])
def test_both_widths_pack_and_unpack_strided_host_rows(lib, cls, dtype, Ks):
    """the packing both indexes share (pq_pack_dword, the host unpack, pq_decode_kernel): M = 3 fills neither a dword of four
    bytes nor one of two uint16, the rows straddle a 64-row block, the host rows lie M + 2 codes apart"""
    n, M, L = 130, 3, 2
    rng = np.random.default_rng(Ks)
    C = rng.standard_normal((M, Ks, L)).astype(np.float32)
    codes = rng.integers(0, Ks, size=(n, M)).astype(dtype)
    codes[0], codes[n - 1] = Ks - 1, Ks - 1                             # the highest codeword is in use
    q = rng.standard_normal((3, M * L)).astype(np.float32)
    wide = np.full((n, M + 2), np.iinfo(dtype).max, dtype)              # what lies between the rows is >= ks
    wide[:, :M] = codes
    with getattr(lib, cls).from_codes(C, wide[:, :M]) as g:
        assert np.array_equal(g.get_codes(60, 10), codes[60:70]) and np.array_equal(g.get_codes(), codes)
        rows = np.concatenate([C[j][codes[60:70, j]] for j in range(M)], axis=1)
        assert np.array_equal(_bits(g.decode(60, 10)), _bits(rows))
        assert _same(g.search(q, n), pq_truth(q, C, codes, n))


def test_ties_come_back_in_ascending_id(lib):
    M, Ks, L = 3, 300, 2
    C, _, q = _problem(700, M, Ks, L, 5)
    one = np.tile(np.array([[299, 7, 256]], np.uint16), (700, 1))
    with lib.WidePQIndex.from_codes(C, one, row_offset=11) as g:       # the tie class is all of N
        ids, dist, _ = g.search(q, 700)
        assert np.array_equal(ids, np.tile(np.arange(11, 711), (5, 1)))
        assert _same((ids, dist), pq_truth(q, C, one, 700, row_offset=11))
    dup = np.repeat(_problem(100, M, Ks, L, 5)[1], 7, axis=0)           # every code seven times
    with lib.WidePQIndex.from_codes(C, dup) as g:
        assert _same(g.search(q, 100), pq_truth(q, C, dup, 100))


def test_allow_bitmaps(lib):
    n, M, Ks, L, K = 5000, 16, 8192, 1, 100
    C, codes, q = _problem(n, M, Ks, L, 1)
    q = np.concatenate([q, q[::-1] * 0.5, q * 2.0])
    rng = np.random.default_rng(4)
    mask = rng.random(n) < 0.4
    few = np.sort(rng.choice(n, 37, replace=False))
    with lib.WidePQIndex.from_codes(C, codes, row_offset=1000) as g:
        assert _same(g.search(q, K, allow=mask), pq_truth(q, C, codes, K, 1000, mask))
        ids = (np.flatnonzero(mask) + 1000).astype(np.int64)
        assert _same(g.search(q, K, allow=ids), pq_truth(q, C, codes, K, 1000, mask))
        fm = np.zeros(n, bool)
        fm[few] = True
        got = g.search(q, K, allow=few + 1000)                          # fewer admitted rows than K
        assert _same(got, pq_truth(q, C, codes, K, 1000, fm))
        assert (got[0][:, 37:] == -1).all() and np.isposinf(got[1][:, 37:]).all()
        got = g.search(q, K, allow=np.zeros(n, bool))                   # none admitted
        assert (got[0] == -1).all() and np.isposinf(got[1]).all()


def test_device_codes_with_a_wide_stride(lib):
    import torch
    n, M, Ks, L, K = 1000, 5, 300, 2, 50
    C, codes, q = _problem(n, M, Ks, L, 6)
    stride = M + 4
    wide = np.full((n, stride), 0xFFFF, np.uint16)                      # 0xFFFF between the rows
    wide[:, M + 1] = 300                                                # ... and a value >= Ks there
    wide[:, :M] = codes
    dev = torch.from_numpy(wide.view(np.int16)).cuda()
    torch.cuda.synchronize()
    want = pq_truth(q, C, codes, K)
    with lib.WidePQIndex.from_device_ptr(C, dev.data_ptr(), n, row_stride=stride) as g:
        assert _same(g.search(q, K), want)
        assert np.array_equal(g.get_codes(), codes)
    with lib.WidePQIndex.from_codes(C, wide[:, :M]) as g:               # the host form of the same stride
        assert _same(g.search(q, K), want)
    bad = wide.copy()
    bad[n - 1, M - 1] = 300
    dev = torch.from_numpy(bad.view(np.int16)).cuda()
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="a code is >= ks"):
        lib.WidePQIndex.from_device_ptr(C, dev.data_ptr(), n, row_stride=stride)
    with lib.WidePQIndex.empty(C, 2 * n) as g:                          # a refused append leaves the index as it was
        g.append_codes(codes)
        with pytest.raises(RuntimeError, match="a code is >= ks"):
            lib.check(lib.load().mi_pqw_append_codes(g._h, dev.data_ptr(), n, stride, lib.MI_DEVICE))
        assert _same(g.search(q, K), want)


@pytest.mark.parametrize("M,Ks,L", [(3, 257, 5), (2, 300, 70), (1, 8192, 2), (16, 4096, 1)])
def test_encoder_is_the_truth(lib, M, Ks, L):
    rng = np.random.default_rng(M + Ks + L)
    C = rng.standard_normal((M, Ks, L)).astype(np.float32)
    C[:, Ks - 1] = C[:, 5]                                              # duplicate codewords: the lower one wins
    C[:, 40] = C[:, 17]
    n = 700
    x64 = rng.standard_normal((n, M * L))
    pick = rng.integers(0, Ks, size=(n, M))
    x64[:200] = np.concatenate([C[j][pick[:200, j]] for j in range(M)], axis=1)        # rows that ARE codewords
    x64[:50] = np.concatenate([C[j][np.full(50, 40)] for j in range(M)], axis=1)       # ... the duplicated ones among them
    x64[50:100] = np.concatenate([C[j][np.full(50, Ks - 1)] for j in range(M)], axis=1)
    x32 = x64.astype(np.float32)
    want32, want64 = encode_truth16(x32, C), encode_truth16(x64, C)
    assert (want32[:50] == 17).all() and (want32[50:100] == 5).all()
    strided = np.full((n, 2 * M * L + 3), 1e30, np.float32)
    strided[:, 0:2 * M * L:2] = x32
    with lib.WidePQIndex.empty(C, 2 * n) as g:
        assert np.array_equal(g.encode(x32), want32) and g.encode(x32).dtype == np.uint16
        assert np.array_equal(g.encode(x64), want64)
        assert np.array_equal(g.encode(strided[:, 0:2 * M * L:2]), want32)
        assert np.array_equal(g.encode(np.asfortranarray(x64)), want64)
        g.add(x32)
        g.add(x64)
        assert g.n == 2 * n and np.array_equal(g.get_codes(), np.concatenate([want32, want64]))
        rows = np.concatenate([C[j][want32[:, j]] for j in range(M)], axis=1)          # decode(get_codes()) is the codebook rows
        assert np.array_equal(_bits(g.decode(0, n)), _bits(rows))


@functools.lru_cache(maxsize=None)
def _training(n, M, Ks, L, iters, kind):
    rng = np.random.RandomState(n + 7 * M + Ks + 3 * L)
    if kind == "clustered":
        x, init = clustered(rng, n, M, Ks, L)
        init[:, Ks - 1] = init[:, 3]                                    # two codewords start from one row: ties go to the lower, so
        init[:, 150] = init[:, 149]                                     # the upper has no member in the first update
    else:
        x = rng.randn(n, M * L).astype(np.float32)
        init = np.stack([rng.choice(n, Ks, replace=False) for _ in range(M)])
    C0 = rows_init(x, M, init)
    C, moved, emptied = train_truth16(x, M, Ks, iters, C0)
    for a in (x, init, C0, C, moved):
        a.setflags(write=False)
    return x, init, C0, C, moved, emptied


TRAIN = [(600, 2, 300, 4, 4, "random"), (9000, 3, 4096, 5, 2, "random"), (8192, 1, 8192, 2, 3, "random"),
         (2000, 2, 300, 3, 4, "clustered")]


@pytest.mark.parametrize("n,M,Ks,L,iters,kind", TRAIN)
def test_training_is_the_truth_and_scipy_bit_for_bit(lib, n, M, Ks, L, iters, kind):
    vq = pytest.importorskip("scipy.cluster.vq")
    x, init, C0, want, moved, emptied = _training(n, M, Ks, L, iters, kind)
    print("codewords without members over the run:", emptied)
    if kind == "clustered":
        assert emptied > 0                                              # the case an update kernel gets wrong
    got, got_moved = lib.pqw_train(x, M, Ks, iters=iters, init=C0)
    assert got.dtype == np.float32 and got.shape == (M, Ks, L)
    assert np.array_equal(got_moved, moved), (got_moved, moved)
    assert np.array_equal(_bits(got), _bits(want))
    import warnings
    for j in range(M):
        xj = x[:, j * L:(j + 1) * L].astype(np.float64)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                             # scipy warns of the empty clusters
            cent, _ = vq.kmeans2(xj, xj[init[j]], iter=iters, minit="matrix")
        assert np.array_equal(_bits(cent.astype(np.float32)), _bits(got[j])), j


def test_training_resumes_stops_and_equals_the_byte_trainer(lib):
    n, M, Ks, L, iters, kind = TRAIN[0]
    x, init, C0, want, moved, _ = _training(n, M, Ks, L, iters, kind)
    for i in (1, 3):
        head, m0 = lib.pqw_train(x, M, Ks, iters=i, init=C0)
        tail, m1 = lib.pqw_train(x, M, Ks, iters=iters - i, init=head)
        assert np.array_equal(_bits(tail), _bits(want)) and np.array_equal(m0, moved[:i])
        assert np.array_equal(m1[1:], moved[i + 1:])                    # (the first count of a run is n * M by definition)
    # early stop: run to the fixed point, the remaining counts are zero and the codebooks those of the last update
    long, lm = lib.pqw_train(x, M, Ks, iters=60, init=C0)
    stop = int(np.flatnonzero(lm == 0)[0])
    assert stop < 59 and (lm[stop:] == 0).all() and (lm[:stop] > 0).all()
    again, _ = lib.pqw_train(x, M, Ks, iters=stop, init=C0)
    assert np.array_equal(_bits(long), _bits(again))
    # Ks <= 256: the byte trainer's bits, by init, by seed and by default rows
    xs = x[:, :2 * L]
    for kw in (dict(seed=9), dict(), dict(init=C0[:, :200])):
        a, am = lib.pqw_train(xs, 2, 200, iters=5, **kw)
        b, bm = lib.pq_train(xs, 2, 200, iters=5, **kw)
        assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(am, bm), kw
    import torch
    dev = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    torch.cuda.synchronize()
    got, gm = lib.pqw_train_device(dev.data_ptr(), n, M * L, M, Ks, iters, init=C0)
    assert np.array_equal(_bits(got), _bits(want)) and np.array_equal(gm, moved)


def test_matcher_end_to_end(lib, tmp_path, monkeypatch):
    from isehr_amd import nnsearch
    from isehr_amd.nnsearch import matching_Nano_PQ_wide_hip, Nano_PQ_wide_hip
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(12)
    n, d, M, bits, K = 2000, 16, 4, 9, 20
    train = rng.standard_normal((n, d)) * 3.0
    test = rng.standard_normal((7, d)).astype(np.float32)
    idx, tpq = matching_Nano_PQ_wide_hip(K, train, test, "wide/set", M, bits)
    assert idx.shape == (7, K) and idx.dtype == np.int64 and tpq > 0
    path = os.path.join("outputs", "wide_set", "mi355_pqw_M4_Ks512.npz")
    assert os.path.exists(path) and sorted(os.listdir(os.path.dirname(path))) == ["mi355_pqw_M4_Ks512.npz"]
    tn = (train / np.linalg.norm(train, axis=1, keepdims=True)).astype(np.float32)
    qn = (test / np.linalg.norm(test, axis=1, keepdims=True)).astype(np.float32)
    books, _ = lib.pqw_train(tn, M, 512, iters=20, seed=42)
    with np.load(path) as z:
        assert np.array_equal(_bits(z["codebooks"]), _bits(books))
    codes = encode_truth16(tn, books)
    assert np.array_equal(idx, pq_truth(qn, books, codes, K)[0])
    again, _ = matching_Nano_PQ_wide_hip(K, train, test, "wide/set", M, bits, ifgenerate=False)
    assert np.array_equal(again, idx)
    with pytest.raises(FileNotFoundError):
        matching_Nano_PQ_wide_hip(K, train, test, "another/set", M, bits, ifgenerate=False)
    assert nnsearch.MATCHING_METHODS["PQ13"] is matching_Nano_PQ_wide_hip
    got_codes, codewords, recon = Nano_PQ_wide_hip(train, M, 512)
    assert got_codes.dtype == np.uint16 and np.array_equal(got_codes, codes)
    assert codewords.shape == (512, d) and np.array_equal(_bits(recon), _bits(np.concatenate([books[j][codes[:, j]] for j in range(M)], axis=1)))


def test_refine_returns_what_the_gallery_returns_for_the_shortlist(lib):
    n, M, Ks, L, K, f = 3000, 4, 300, 4, 10, 8
    rng = np.random.default_rng(21)
    rows = rng.standard_normal((n, M * L)).astype(np.float32)
    q = rng.standard_normal((9, M * L)).astype(np.float32)
    C = rows_init(rows, M, np.stack([rng.choice(n, Ks, replace=False) for _ in range(M)]))
    mask = rng.random(n) < 0.5
    with lib.Gallery.l2_from_host(rows) as raw, lib.WidePQIndex.empty(C, n) as g:
        g.add(rows)
        for kw in ({}, {"allow": mask}):
            short = g.search(q, K * f, **kw)[0]
            want = raw.refine(q, short, K)
            got = g.search(q, K, refine=raw, k_factor=f, **kw)
            assert np.array_equal(got[0], want[0]) and np.array_equal(_bits(got[1]), _bits(want[1])), kw


def test_scratch_is_grow_only_and_returned(lib):
    import torch
    n, M, Ks, L = 200000, 16, 300, 1
    C, codes, q = _problem(n, M, Ks, L, 70)
    allow = np.random.default_rng(2).random(n) < 0.5

    def cycle(check=False):
        with lib.WidePQIndex.from_codes(C, codes) as g:
            base = g.hbm_bytes
            assert base >= (n + 63) // 64 * 64 * 4 * ((M + 1) // 2) + C.size * 4
            g.search(q, 10, allow=allow)
            first = g.hbm_bytes
            g.search(q, 10, allow=allow)
            if check:
                assert first > base + 70 * n * 4 and g.hbm_bytes == first       # a second search of the same shape allocates nothing
                g.search(q[:3], 5)
                assert g.hbm_bytes == first                                     # ... nor does a smaller one

    cycle(check=True)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(6):
        cycle()
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    print("free before / after 6 cycles", free0, free1)
    assert free0 - free1 < 32 * 2**20, (free0, free1)                           # the matrix alone is 56 MB a cycle
