"""CPU: the residual IVF-PQ index (mi_ivfpq_create_residual, mi_ivfpq_is_residual, mi_ivfpq_residual_rows; IVFPQIndex(by_residual=True);
knn.ANN) is exported and bound and answers bad arguments before a device is touched; the numpy truth
(tests/_ivfpq_residual_truth.py) agrees with a literal triple-loop restatement of the contract; and on the clustered fixture of the
issue the truth of the residual index reconstructs strictly better than the truth of the plain one."""
import ctypes as C

import numpy as np
import pytest

from _ivfpq_residual_truth import (reconstruct, residual_encode_truth, residual_ivfpq_truth, residual_rows_truth)
from _ivfpq_truth import ivfpq_truth, probe_truth
from _pq_train_truth import rows_init, train_truth
from _pq_truth import encode_truth

NEW = {"mi_ivfpq_create_residual": 15, "mi_ivfpq_is_residual": 2, "mi_ivfpq_residual_rows": 10, "mi_ivfpq_search_stages_device": 10}


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__
    __graft_entry__.build()
    from isehr_amd import _lib
    return _lib.load(), _lib


def test_symbols_are_declared_exported_and_bound(built_lib):
    import inspect
    import os
    lib, _lib = built_lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mi355_retrieval.h")).read()
    for name, nargs in NEW.items():
        assert "int %s(" % name in header, name
        assert hasattr(lib, name), name
        assert getattr(lib, name).restype == C.c_int
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
    assert _lib.SIGNATURES["mi_ivfpq_create_residual"] == _lib.SIGNATURES["mi_ivfpq_create"]
    IV = _lib.IVFPQIndex
    for meth in ("from_codes", "from_device_ptr", "empty", "fit", "train"):
        assert inspect.signature(getattr(IV, meth)).parameters["by_residual"].default is False, meth
    assert isinstance(IV.by_residual, property) and callable(IV.residual_rows) and callable(IV.search_stages_device)
    from isehr_amd import knn
    sig = inspect.signature(knn.ANN.__init__).parameters
    assert [(p, sig[p].default) for p in ("method", "M", "nbits", "nlist", "nprobe", "seed")] == [
        ("method", "euclidean"), ("M", 64), ("nbits", 8), ("nlist", 256), ("nprobe", 64), ("seed", 0)]


def test_invalid_arguments_answer_without_a_device(built_lib):
    lib, _lib = built_lib
    P = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    rng = np.random.default_rng(0)
    cb = rng.standard_normal((4, 16, 2)).astype(np.float32)                 # m = 4, ks = 16, L = 2, d = 8
    G = rng.standard_normal((5, 8)).astype(np.float32)                      # nlist = 5
    big = np.zeros(257 * 4100, np.float32)
    codes = np.zeros((3, 4), np.uint8)
    lists = np.zeros(3, np.uint8)
    h = C.c_void_p()

    def create(gp=None, nlist=5, cbp=None, d=8, m=4, ks=16, cd=P(codes), li=P(lists), n=3, stride=4, cap=0, out=C.byref(h)):
        return lib.mi_ivfpq_create_residual(P(G) if gp is None else gp, nlist, P(cb) if cbp is None else cbp, d, m, ks, cd, li, n,
                                            stride, _lib.MI_HOST, 0, 0, cap, out)

    # the cases, and the words, of mi_ivfpq_create (tests/test_ivfpq_cpu.py): the same checks in the same order
    cases = [(dict(out=None), b"out"), (dict(nlist=1), b"nlist (lists)"), (dict(nlist=257, gp=P(big)), b"nlist (lists)"),
             (dict(m=0, cbp=P(big)), b"m (books)"), (dict(m=65, d=130, cbp=P(big), gp=P(big)), b"m (books)"),
             (dict(ks=1), b"ks (codewords"), (dict(ks=257, cbp=P(big)), b"ks (codewords"),
             (dict(d=9, cbp=P(big), gp=P(big)), b"multiple of m"), (dict(d=4100, cbp=P(big), gp=P(big)), b"d must be in"),
             (dict(d=0), b"d must be in"), (dict(cap=2), b"capacity"), (dict(cap=-1), b"capacity"),
             (dict(n=-1), b"negative number of rows"), (dict(cd=None), b"codes"), (dict(li=None), b"list_ids"),
             (dict(cd=None, li=None, n=0), b"capacity"), (dict(stride=3), b"row_stride_bytes"),
             (dict(nlist=1, m=0), b"nlist (lists)"), (dict(m=0, ks=1, cbp=P(big)), b"m (books)")]          # the order of the checks
    for kwargs, word in cases:
        assert create(**kwargs) == _lib.MI_ERR_INVALID, kwargs
        assert word in lib.mi_last_error(), (kwargs, lib.mi_last_error())
    assert lib.mi_ivfpq_create_residual(None, 5, P(cb), 8, 4, 16, P(codes), P(lists), 3, 4, _lib.MI_HOST, 0, 0, 0,
                                        C.byref(h)) == _lib.MI_ERR_INVALID
    assert b"coarse_host" in lib.mi_last_error()
    assert lib.mi_ivfpq_create_residual(P(G), 5, None, 8, 4, 16, P(codes), P(lists), 3, 4, _lib.MI_HOST, 0, 0, 0,
                                        C.byref(h)) == _lib.MI_ERR_INVALID
    assert b"codebooks_host" in lib.mi_last_error()
    bad_G = G.copy()
    bad_G[4, 7] = np.inf
    assert create(gp=P(bad_G)) == _lib.MI_ERR_INVALID and b"coarse centroids must be finite" in lib.mi_last_error()
    bad_cb = cb.copy()
    bad_cb[3, 15, 1] = np.nan
    assert create(cbp=P(bad_cb)) == _lib.MI_ERR_INVALID and b"codebooks must be finite" in lib.mi_last_error()
    bad_codes = codes.copy()
    bad_codes[2, 3] = 16
    assert create(cd=P(bad_codes)) == _lib.MI_ERR_INVALID and b">= ks" in lib.mi_last_error()
    bad_lists = lists.copy()
    bad_lists[2] = 5
    assert create(li=P(bad_lists)) == _lib.MI_ERR_INVALID and b">= nlist" in lib.mi_last_error()
    assert h.value is None

    fake = C.c_void_p(16)                         # non-null, never dereferenced: these checks answer before the handle is read
    kind = C.c_int32(7)
    assert lib.mi_ivfpq_is_residual(None, C.byref(kind)) == _lib.MI_ERR_INVALID and b"null handle" in lib.mi_last_error()
    assert lib.mi_ivfpq_is_residual(fake, None) == _lib.MI_ERR_INVALID and b"out" in lib.mi_last_error()
    assert kind.value == 7

    x = np.zeros((2, 8), np.float32)
    out = np.zeros((2, 8), np.float32)

    def rows(hh=fake, xp=P(x), n=2, dtype=_lib.MI_F32, rs=8, cs=1, memspace=_lib.MI_HOST, op=P(out), omem=_lib.MI_HOST):
        return lib.mi_ivfpq_residual_rows(hh, xp, n, dtype, rs, cs, memspace, None, op, omem)

    for kwargs, word in [(dict(hh=None), b"null handle"), (dict(n=-1), b"negative number of rows"), (dict(xp=None), b"null pointer: rows"),
                         (dict(dtype=7), b"dtype"), (dict(rs=-1), b"negative strides"), (dict(cs=-1), b"negative strides"),
                         (dict(memspace=5), b"memspace must be"), (dict(op=None), b"null pointer: out"),
                         (dict(omem=5), b"out_memspace must be")]:
        assert rows(**kwargs) == _lib.MI_ERR_INVALID, kwargs
        assert word in lib.mi_last_error(), (kwargs, lib.mi_last_error())

    idx = np.zeros(8, np.int64)
    t, u = C.c_float(-1.0), C.c_float(-1.0)

    def stages(hh=fake, qp=P(x), nq=2, k=4, nprobe=3, op=P(idx), tp=C.byref(t), up=C.byref(u)):
        return lib.mi_ivfpq_search_stages_device(hh, qp, nq, k, nprobe, op, None, None, tp, up)

    for kwargs, word in [(dict(hh=None), b"null handle"), (dict(k=0), b"k must"), (dict(k=2049), b"k must"), (dict(nq=-1), b"nq must"),
                         (dict(nprobe=0), b"nprobe must"), (dict(nprobe=257), b"nprobe must"), (dict(qp=None), b"null pointer"),
                         (dict(op=None), b"null pointer"), (dict(tp=None), b"out_table_ms"), (dict(up=None), b"out_table_ms")]:
        assert stages(**kwargs) == _lib.MI_ERR_INVALID, kwargs
        assert word in lib.mi_last_error(), (kwargs, lib.mi_last_error())
    assert t.value == -1.0 and u.value == -1.0


def test_wrappers_reject_bad_input_before_the_device(built_lib):
    _, _lib = built_lib
    from isehr_amd.knn import ANN
    rng = np.random.default_rng(1)
    db = rng.standard_normal((40, 8)).astype(np.float32)
    with pytest.raises(ValueError, match="M = 65 books.*1 .. 64"):
        ANN(db, M=65)
    with pytest.raises(ValueError, match="M = 128 books"):
        ANN(db, M=128)                                                   # the reference's default
    with pytest.raises(ValueError, match="nlist = 316 lists.*2 .. 256"):
        ANN(db, nlist=316)                                               # the reference's default
    with pytest.raises(ValueError, match="nlist = 257"):
        ANN(db, nlist=257)
    with pytest.raises(ValueError, match="nbits = 4.*nbits = 8 only"):
        ANN(db, nbits=4)
    with pytest.raises(ValueError, match="nprobe = 9"):
        ANN(db, M=4, nlist=8, nprobe=9)
    with pytest.raises(ValueError, match="no multiple of M"):
        ANN(db, M=3, nlist=8, nprobe=2)
    with pytest.raises(NotImplementedError):
        ANN(db, method="hamming")
    with pytest.raises(ValueError, match="training rows"):
        ANN(db, M=4, nlist=8, nprobe=2)                                  # 40 // 5 = 8 rows cannot seed 256 codewords
    IV = _lib.IVFPQIndex
    books = rng.standard_normal((4, 16, 2)).astype(np.float32)
    G = rng.standard_normal((5, 8)).astype(np.float32)
    codes = rng.integers(0, 16, size=(40, 4))
    lists = rng.integers(0, 5, size=40)
    with pytest.raises(ValueError, match="nlist = 257"):
        IV.from_codes(np.zeros((257, 8), np.float32), books, codes, lists, by_residual=True)
    with pytest.raises(ValueError, match=r"\[0, nlist = 5\)"):
        IV.from_codes(G, books, codes, lists + 1, by_residual=True)
    with pytest.raises(ValueError, match="capacity"):
        IV.empty(G, books, 0, by_residual=True)
    with pytest.raises(ValueError, match="nlist = 300"):
        IV.fit(db, 300, 4, 16, by_residual=True)
    with pytest.raises(ValueError, match="nlist = 1 "):
        IV.train(db, 1, 4, 16, by_residual=True)
    idx = IV.__new__(IV)
    idx._h, idx.n, idx.d, idx.m, idx.ks, idx.nlist, idx.row_offset = None, 40, 8, 4, 16, 5, 0
    with pytest.raises(ValueError, match="rows of 4 columns"):
        idx.residual_rows(db[:, :4])
    with pytest.raises(ValueError, match=r"\[0, nlist = 5\)"):
        idx.residual_rows(db, lists + 1)
    with pytest.raises(ValueError, match=r"list ids must be \[rows = 40\]"):
        idx.residual_rows(db, lists[:39])


def _loops(x, G, C, codes, lists, probes, k):
    """The contract, literally: per query, per distinct probed list, per row of that list, per book, per column."""
    M, Ks, L = C.shape
    ids, dist = [], []
    for q in range(x.shape[0]):
        cand = []
        for l in sorted({int(p) for p in probes[q] if p >= 0}):
            r = [np.float64(x[q, j]) - np.float64(G[l, j]) for j in range(M * L)]
            T = np.zeros((M, Ks), np.float32)
            for m in range(M):
                for c in range(Ks):
                    acc = np.float64(0.0)
                    for j in range(L):
                        t = r[m * L + j] - np.float64(C[m, c, j])
                        acc = acc + t * t
                    T[m, c] = np.float32(acc)
            for i in np.flatnonzero(lists == l):
                s = np.float32(0.0)
                for m in range(M):
                    s = np.float32(s + T[m, codes[i, m]])
                cand.append((s, int(i)))
        cand.sort()
        cand = cand[:k] + [(np.float32(np.inf), -1)] * (k - len(cand[:k]))
        ids.append([c[1] for c in cand])
        dist.append([c[0] for c in cand])
    return np.array(ids, np.int64), np.array(dist, np.float32)


def test_truth_agrees_with_a_triple_loop_on_a_tiny_case():
    rng = np.random.default_rng(7)
    M, Ks, L, nlist, n, nq = 3, 5, 2, 4, 30, 4
    Cb = rng.standard_normal((M, Ks, L)).astype(np.float32)
    G = (3 * rng.standard_normal((nlist, M * L))).astype(np.float32)
    codes = rng.integers(0, Ks, size=(n, M), dtype=np.uint8)
    lists = rng.integers(0, nlist - 1, size=n).astype(np.uint8)           # list 3 is empty
    codes[7], lists[7], lists[2] = codes[2], 0, 1                         # the same code in two lists
    x = rng.standard_normal((nq, M * L))
    probes = np.array([[0, 1, 2], [3, -1, 3], [2, 2, 0], [1, -1, -1]])
    got = residual_ivfpq_truth(x, G, Cb, codes, lists, probes, 40)
    want = _loops(x, G, Cb, codes, lists, probes, 40)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    assert (got[0][1] == -1).all()                                        # an empty list and "no list"
    # rows 2 and 7 share their code bytes and differ in their list: their distances differ
    d = dict(zip(got[0][0].tolist(), got[1][0].tolist()))
    assert d[2] != d[7]
    # zero centroids: the plain truth
    Z = np.zeros_like(G)
    plain = ivfpq_truth(x, Cb, codes, lists, probes, 40)
    zero = residual_ivfpq_truth(x, Z, Cb, codes, lists, probes, 40)
    assert np.array_equal(zero[0], plain[0]) and np.array_equal(zero[1].view(np.uint32), plain[1].view(np.uint32))
    # the encoder: lists by the nearest centroid, codes of the float64 residual
    xs = (G[rng.integers(0, nlist, size=20)] + 0.5 * rng.standard_normal((20, M * L))).astype(np.float32)
    cd, li = residual_encode_truth(xs, G, Cb)
    assert np.array_equal(li, probe_truth(xs, G, 1)[:, 0])
    for i in range(20):
        r = xs[i].astype(np.float64) - G[li[i]].astype(np.float64)
        for m in range(M):
            sums = [sum((r[m * L + j] - np.float64(Cb[m, c, j])) ** 2 for j in range(L)) for c in range(Ks)]
            assert cd[i, m] == int(np.argmin(sums))
    assert np.array_equal(residual_rows_truth(xs, G, li), (xs.astype(np.float64) - G[li].astype(np.float64)).astype(np.float32))


def quality_fixture(i=0):
    """The clustered fixture of the quality condition, drawn by RandomState(100 + i)."""
    rs = np.random.RandomState(100 + i)
    n, d, nc = 2048, 32, 8
    cen = rs.randn(nc, d) * 3
    return np.float32(cen[rs.randint(nc, size=n)] + 0.3 * rs.randn(n, d))


QUALITY = dict(nlist=8, M=4, Ks=16, seed=42)


def quality_truth(x, nlist, M, Ks, seed, iters=20):
    """What IVFPQIndex.fit computes, with and without residuals, by the numpy truths and the project's initial-row rule (one
    RandomState(seed) per pq_train call: `choice(n, Ks)` once per book).  -> (G, (C, codes, lists) plain, (C, codes, lists)
    residual)"""
    n = x.shape[0]
    G = train_truth(x, 1, nlist, iters, rows_init(x, 1, np.random.RandomState(seed).choice(n, nlist, replace=False)[None]))[0][0]
    rng = np.random.RandomState(seed)
    rows = np.stack([rng.choice(n, Ks, replace=False) for _ in range(M)])
    lists = probe_truth(x, G, 1)[:, 0].astype(np.uint8)
    Cp = train_truth(x, M, Ks, iters, rows_init(x, M, rows))[0]
    res = residual_rows_truth(x, G, lists)
    Cr = train_truth(res, M, Ks, iters, rows_init(res, M, rows))[0]
    return G, (Cp, encode_truth(x, Cp), lists), (Cr,) + residual_encode_truth(x, G, Cr)


def mse(x, G, C, codes, lists, by_residual):
    return float(((x.astype(np.float64) - reconstruct(G, C, codes, lists, by_residual)) ** 2).sum(1).mean())


def test_quality_condition_holds_for_the_truth():
    """RandomState(100) itself satisfies the condition under the project's initial-row rule (no later draw was needed): the truth
    gives 1.9548 with residuals against 7.1302 without."""
    x = quality_fixture(0)
    G, plain, resid = quality_truth(x, **QUALITY)
    e_plain, e_resid = mse(x, G, *plain, False), mse(x, G, *resid, True)
    print("mean squared reconstruction error: plain %.6f residual %.6f" % (e_plain, e_resid))
    assert e_resid < e_plain
