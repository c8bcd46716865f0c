"""GPU: the IVF-Flat index (mi_ivfflat*, IVFFlatIndex, matching_IVF_hip) against the truth of
tests/_ivfflat_truth.py bit for bit on lattice data (integer-valued float32 in [-3, 3]: every float64 sum is exact in any order, and
the tie classes are large), against Gallery.search_l2 with the allow bitmap of the probed lists, against the exhaustive search with
nprobe == nlist, and against Gallery.refine over the lists' rows on an inner-product gallery."""
import numpy as np
import pytest

import _ivfflat_truth as T
from _graph_truth import gallery_rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from isehr_amd import _lib
    _lib.load()
    return _lib


def _gallery(lib, rows, kind, off=0, capacity=0):
    if kind == "l2":
        return lib.Gallery.l2_from_host(rows, row_offset=off, capacity=capacity)
    return lib.Gallery.from_host(rows, norm_mode=lib.NORM_NONE, row_offset=off)


def _mask(cand, n):
    m = np.zeros(n, bool)
    m[cand] = True
    return m


def _check(lib, g, f, q, k, l2, nprobe=1, probes=None, allow=None, references=True):
    """f.search == the truth bit for bit (ids, float64 values, their float32 cast, the rows evaluated); on an L2 gallery also ==
    Gallery.search_l2 with the allow bitmap of each query's candidates; on any other == Gallery.refine over them where they number
    <= 8192."""
    stored = gallery_rows(g)
    off, lr = f.lists()
    used = f.probe(q, nprobe) if probes is None else np.asarray(probes)
    if probes is None:
        assert np.array_equal(used, T.probe(q, f.centroids(), nprobe, l2))
    ids, v64, secs, scanned = f.search(q, k, nprobe=nprobe, probes=probes, allow=allow, return_values64=True, return_scanned=True)
    _, v32, _ = f.search(q, k, nprobe=nprobe, probes=probes, allow=allow)
    t_ids, t_val, t_scanned = T.search(q, stored, used, off, lr, f.nlist, k, l2, g.row_offset, allow)
    assert ids.dtype == np.int64 and ids.shape == (len(q), k) and secs > 0
    assert np.array_equal(ids, t_ids)
    assert v64.tobytes() == t_val.tobytes() and v32.tobytes() == t_val.astype(np.float32).tobytes()
    assert np.array_equal(scanned, t_scanned)
    if not references:
        return ids
    cand = T.candidates(used, off, lr, f.nlist, allow)
    for i in range(min(len(q), 4)):
        if l2 and len(cand[i]):
            w_ids, _, w64, _, _ = g.search_l2(q[i:i + 1], k, allow=_mask(cand[i], g.n))
            assert np.array_equal(ids[i:i + 1], w_ids) and v64[i:i + 1].tobytes() == w64.tobytes()
        elif 1 <= len(cand[i]) <= 8192:
            kk = min(k, len(cand[i]))
            w_ids, _, w64, _ = g.refine(q[i:i + 1], (cand[i] + g.row_offset)[None, :], kk)
            assert np.array_equal(ids[i:i + 1, :kk], w_ids) and v64[i:i + 1, :kk].tobytes() == w64.tobytes()
            assert (ids[i, kk:] == -1).all() and (v64[i, kk:] == -np.inf).all()
    return ids


@pytest.mark.parametrize("kind", ["l2", "ip"])
@pytest.mark.parametrize("nlist", [7, 64, 300])
@pytest.mark.parametrize("d", [20, 64])
def test_build_and_search_on_base_shapes(lib, d, nlist, kind):
    rng = np.random.default_rng(1000 * d + nlist)
    n, l2, off = 5000, kind == "l2", 70
    rows, cent, q = T.lattice(rng, (n, d)), T.lattice(rng, (nlist, d)), T.lattice(rng, (9, d))
    g = _gallery(lib, rows, kind, off)
    try:
        with lib.IVFFlatIndex.build(g, cent) as f, lib.IVFFlatIndex.build(g, cent) as f2:
            assert (f.n, f.d, f.nlist) == (n, d, nlist) and f.hbm_bytes >= 4 * n
            assert f.centroids().tobytes() == cent.tobytes()
            lid = T.assign(gallery_rows(g), cent, l2)
            t_off, t_lr = T.lists_of(lid, nlist)
            loff, lrows = f.lists()
            assert loff.dtype == np.int64 and lrows.dtype == np.int32
            assert np.array_equal(loff, t_off) and np.array_equal(lrows, t_lr) and np.array_equal(f.list_ids(), lid)
            assert all((np.diff(lrows[loff[l]:loff[l + 1]]) > 0).all() for l in range(nlist))
            assert np.array_equal(f.list_sizes(), np.diff(t_off))
            o2, r2 = f2.lists()
            assert o2.tobytes() == loff.tobytes() and r2.tobytes() == lrows.tobytes()
            _check(lib, g, f, q, 100, l2, nprobe=min(5, nlist))
            ids = _check(lib, g, f, q[:3], 100, l2, nprobe=nlist, references=False)
            if l2:                                               # every list probed: the exhaustive search, bit for bit
                w_ids, _, w64, _, _ = g.search_l2(q[:3], 100)
                _, v64, _ = f.search(q[:3], 100, nprobe=nlist, return_values64=True)
                assert np.array_equal(ids, w_ids) and v64.tobytes() == w64.tobytes()
    finally:
        g.close()


@pytest.fixture(scope="module")
def skewed(lib):
    """n = 3 S + 700 rows in 6 lists: list 0 empty, list 1 one row, list 2 longer than a slab (S + 300), list 3 of 500 rows, list 4 the
    rest, list 5 of 37 rows, dealt out so that no list is a run of consecutive rows."""
    S = lib.IVFFLAT_SLAB_ROWS
    n, d, nlist = 3 * S + 700, 12, 6
    rng = np.random.default_rng(77)
    sizes = [0, 1, S + 300, 500, n - (1 + S + 300 + 500 + 37), 37]
    lid = rng.permutation(np.repeat(np.arange(nlist), sizes)).astype(np.int32)
    return n, d, nlist, lid, T.lattice(rng, (n, d)), T.lattice(rng, (nlist, d)), T.lattice(rng, (5, d)), sizes


@pytest.mark.parametrize("kind", ["l2", "ip"])
def test_skewed_lists_slab_boundaries_and_edges(lib, skewed, kind):
    n, d, nlist, lid, rows, cent, q, sizes = skewed
    S, l2 = lib.IVFFLAT_SLAB_ROWS, kind == "l2"
    g = _gallery(lib, rows, kind, 11)
    try:
        with lib.IVFFlatIndex.from_lists(g, cent, lid) as f:
            off, lr = f.lists()
            t_off, t_lr = T.lists_of(lid, nlist)
            assert np.array_equal(off, t_off) and np.array_equal(lr, t_lr) and f.list_sizes().tolist() == sizes
            # lists 3, 2, 4: 500 + (S + 300) + the rest -> at least three slabs, the first boundary inside list 2
            span = np.tile(np.array([[3, 2, 4]], np.int32), (len(q), 1))
            assert 500 < S < 500 + sizes[2] and 500 + sizes[2] + sizes[4] > 2 * S
            for k in (1, 100, 2048):
                _check(lib, g, f, q, k, l2, probes=span)
            # k beyond the candidates: the empty list and the list of one row
            ids = _check(lib, g, f, q, 5, l2, probes=np.tile(np.array([[0, 1]], np.int32), (len(q), 1)))
            assert (ids[:, 0] >= 0).all() and (ids[:, 1:] == -1).all()
            ids = _check(lib, g, f, q, 3, l2, probes=np.zeros((len(q), 1), np.int32))
            assert (ids == -1).all()
            # a caller's probes with repeats, -1 and an entry out of range; rows of different lengths of sequence
            messy = np.array([[5, 5, -1, 9, 1], [9, -1, -1, 9, 9], [2, 2, 2, 2, 2], [1, 0, 5, 1, 0], [-1, 3, 6, 3, 5]], np.int32)
            _check(lib, g, f, q, 100, l2, probes=messy)
            # an allow bitmap that empties list 5 entirely and thins the others
            allow = np.random.default_rng(5).random(n) < 0.5
            allow[lid == 5] = False
            ids = _check(lib, g, f, q, 100, l2, probes=np.tile(np.array([[5, 3, 2]], np.int32), (len(q), 1)), allow=allow)
            assert not np.isin(ids - g.row_offset, np.flatnonzero(lid == 5)).any()
            ids = _check(lib, g, f, q, 4, l2, probes=np.full((len(q), 1), 5, np.int32), allow=allow)
            assert (ids == -1).all()
            # the library's probes over every list
            _check(lib, g, f, q[:2], 2048, l2, nprobe=nlist)
            # nq = 0
            ids, vals, _ = f.search(np.zeros((0, d), np.float32), 3)
            assert ids.shape == (0, 3) and vals.shape == (0, 3)
            assert f.probe(np.zeros((0, d), np.float32), 2).shape == (0, 2)
            for bad in (0, nlist + 1):
                with pytest.raises(ValueError, match="nprobe"):
                    f.search(q, 3, nprobe=bad)
            rc = lib.load().mi_ivfflat_search_device(f._h, 16, len(q), 3, nlist + 1, None, None, 16, None, None, None, None)
            assert rc == lib.MI_ERR_INVALID and b"nprobe" in lib.load().mi_last_error()
    finally:
        g.close()


def test_create_refuses_bad_centroids_and_list_ids(lib):
    import ctypes as C
    import torch
    rng = np.random.default_rng(3)
    rows, cent = T.lattice(rng, (100, 6)), T.lattice(rng, (4, 6))
    with lib.Gallery.l2_from_host(rows) as g:
        out = C.c_void_p()
        bad_c = cent.copy()
        bad_c[2, 5] = np.inf
        assert lib.load().mi_ivfflat_build(g._h, bad_c.ctypes.data, 4, C.byref(out)) == lib.MI_ERR_INVALID
        assert b"finite" in lib.load().mi_last_error()
        for value in (4, -1):
            lid = np.zeros(100, np.int32)
            lid[57] = value
            assert lib.load().mi_ivfflat_create(g._h, cent.ctypes.data, 4, lid.ctypes.data, lib.MI_HOST, C.byref(out)) == lib.MI_ERR_INVALID
            assert b"list ids" in lib.load().mi_last_error()
            dev = torch.from_numpy(lid).cuda()                    # the flag kernel of the device path
            assert lib.load().mi_ivfflat_create(g._h, cent.ctypes.data, 4, dev.data_ptr(), lib.MI_DEVICE, C.byref(out)) == lib.MI_ERR_INVALID
            assert b"list ids" in lib.load().mi_last_error()
        assert out.value is None
        lid = rng.integers(0, 4, 100).astype(np.int32)
        dev = torch.from_numpy(lid).cuda()
        lib.check(lib.load().mi_ivfflat_create(g._h, cent.ctypes.data, 4, dev.data_ptr(), lib.MI_DEVICE, C.byref(out)))
        with lib.IVFFlatIndex(out.value, g) as f, lib.IVFFlatIndex.from_lists(g, cent, lid) as f2:
            assert np.array_equal(f.list_ids(), lid) and f.lists()[1].tobytes() == f2.lists()[1].tobytes()


def test_more_queries_than_one_grid_holds(lib):
    rng = np.random.default_rng(9)
    n, d, nlist, nq = 256, 4, 5, 65538
    rows, cent, q = T.lattice(rng, (n, d)), T.lattice(rng, (nlist, d)), T.lattice(rng, (nq, d))
    with lib.Gallery.l2_from_host(rows) as g, lib.IVFFlatIndex.build(g, cent) as f:
        ids, v64, _, scanned = f.search(q, 3, nprobe=2, return_values64=True, return_scanned=True)
        off, lr = f.lists()
        pick = np.r_[0:40, 65500:65538]                          # both sides of the 65535-query chunk
        t_ids, t_val, t_scanned = T.search(q[pick], rows, T.probe(q[pick], cent, 2, True), off, lr, nlist, 3, True)
        assert np.array_equal(ids[pick], t_ids) and v64[pick].tobytes() == t_val.tobytes()
        assert np.array_equal(scanned[pick], t_scanned)
        # a query's answer does not depend on the batch it came in: equal queries, equal answers
        _, first = np.unique(q, axis=0, return_index=True)
        inv = {tuple(q[i]): i for i in first}
        same = np.array([inv[tuple(r)] for r in q[65000:]])
        assert np.array_equal(ids[65000:], ids[same]) and v64[65000:].tobytes() == v64[same].tobytes()


@pytest.mark.parametrize("kind", ["l2", "ip"])
def test_device_form_equals_host_form_and_reuses_its_scratch(lib, kind):
    import torch
    rng = np.random.default_rng(21)
    n, d, nlist, k, nprobe = 3000, 10, 9, 50, 4
    rows, cent, q = T.lattice(rng, (n, d)), T.lattice(rng, (nlist, d)), T.lattice(rng, (40, d))
    allow = rng.random(n) < 0.7
    g = _gallery(lib, rows, kind, 5)
    try:
        with lib.IVFFlatIndex.build(g, cent) as f:
            s = torch.cuda.current_stream().cuda_stream
            bits = torch.from_numpy(np.asarray(lib.allow_bitmap(allow, n)).view(np.int64)).cuda()
            probes = rng.integers(-1, nlist + 1, (40, nprobe)).astype(np.int32)
            for nq, pr, al in ((40, None, None), (7, None, allow), (40, probes, allow), (3, probes, None)):
                tq = torch.from_numpy(q[:nq]).cuda()
                didx = torch.full((nq, k), -7, dtype=torch.int64, device="cuda")
                dv32 = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
                dv64 = torch.zeros((nq, k), dtype=torch.float64, device="cuda")
                dsc = torch.full((nq,), -7, dtype=torch.int64, device="cuda")
                tp = None if pr is None else torch.from_numpy(pr[:nq]).cuda()
                f.search_device(tq.data_ptr(), nq, k, didx.data_ptr(), val_ptr=dv32.data_ptr(), val64_ptr=dv64.data_ptr(), nprobe=nprobe,
                                probes_ptr=None if tp is None else tp.data_ptr(), allow_ptr=None if al is None else bits.data_ptr(),
                                scanned_ptr=dsc.data_ptr(), stream=s)
                torch.cuda.synchronize()
                ids, v64, _, scanned = f.search(q[:nq], k, nprobe=nprobe, probes=None if pr is None else pr[:nq], allow=al,
                                                return_values64=True, return_scanned=True)
                assert np.array_equal(didx.cpu().numpy(), ids) and dv64.cpu().numpy().tobytes() == v64.tobytes()
                assert dv32.cpu().numpy().tobytes() == v64.astype(np.float32).tobytes()
                assert np.array_equal(dsc.cpu().numpy(), scanned)
            # two batch sizes on one handle: the answers of the shared queries are equal
            a = f.search(q, k, nprobe=nprobe, return_values64=True)
            b = f.search(q[:6], k, nprobe=nprobe, return_values64=True)
            c = f.search(q, k, nprobe=nprobe, return_values64=True)
            assert np.array_equal(a[0][:6], b[0]) and a[1][:6].tobytes() == b[1].tobytes()
            assert np.array_equal(a[0], c[0]) and a[1].tobytes() == c[1].tobytes()
            # ids alone: the value outputs may be NULL
            didx = torch.full((6, k), -7, dtype=torch.int64, device="cuda")
            tq = torch.from_numpy(q[:6]).cuda()
            f.search_device(tq.data_ptr(), 6, k, didx.data_ptr(), nprobe=nprobe, stream=s)
            torch.cuda.synchronize()
            assert np.array_equal(didx.cpu().numpy(), b[0])
    finally:
        g.close()


def test_stale_handle_is_refused(lib):
    rng = np.random.default_rng(4)
    rows, cent, q = T.lattice(rng, (500, 8)), T.lattice(rng, (5, 8)), T.lattice(rng, (2, 8))
    with lib.Gallery.l2_from_host(rows, capacity=600) as g, lib.IVFFlatIndex.build(g, cent) as f:
        f.search(q, 3)
        g.remove(np.array([7, 9]))
        for call in (lambda: f.search(q, 3), lambda: f.probe(q, 2)):
            with pytest.raises(RuntimeError, match="gallery has been appended to or had rows removed"):
                call()
        with lib.IVFFlatIndex.build(g, cent) as f2:
            f2.search(q, 3)
            g.append(rows[:3])
            for call in (lambda: f2.search(q, 3), lambda: f2.probe(q, 2)):
                with pytest.raises(RuntimeError, match="gallery has been appended to or had rows removed"):
                    call()


def test_more_lists_than_refines_small_tier(lib):
    """nlist = 2049: the probe runs in refine's large tier (more than 2048 candidates)."""
    rng = np.random.default_rng(12)
    n, d, nlist = 4000, 8, 2049
    rows, cent, q = T.lattice(rng, (n, d)), T.lattice(rng, (nlist, d)), T.lattice(rng, (4, d))
    with lib.Gallery.l2_from_host(rows) as g, lib.IVFFlatIndex.build(g, cent) as f:
        assert np.array_equal(f.list_ids(), T.assign(rows, cent, True))
        _check(lib, g, f, q, 100, True, nprobe=300)
        _check(lib, g, f, q, 7, True, nprobe=1)


def test_every_one_of_8192_lists_probed(lib):
    rng = np.random.default_rng(13)
    n, d, nlist = 8192, 4, 8192
    rows, cent, q = T.lattice(rng, (n, d)), T.lattice(rng, (nlist, d)), T.lattice(rng, (3, d))
    lid = rng.integers(0, nlist, n).astype(np.int32)
    with lib.Gallery.l2_from_host(rows) as g, lib.IVFFlatIndex.from_lists(g, cent, lid) as f:
        ids = _check(lib, g, f, q, 100, True, nprobe=nlist, references=False)
        w_ids, _, w64, _, _ = g.search_l2(q, 100)
        _, v64, _ = f.search(q, 100, nprobe=nlist, return_values64=True)
        assert np.array_equal(ids, w_ids) and v64.tobytes() == w64.tobytes()


def test_gaussian_rows_against_the_librarys_exact_searches(lib):
    """Not lattice data: the sums round, so only the library's own exact searches are the reference."""
    rng = np.random.default_rng(14)
    n, d, nlist, nprobe, k = 4000, 32, 16, 3, 50
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((6, d)).astype(np.float32)
    cent = lib.IVFFlatIndex.train(rows, nlist)
    assert cent.shape == (nlist, d) and cent.dtype == np.float32
    with lib.Gallery.l2_from_host(rows) as g, lib.IVFFlatIndex.build(g, cent) as f:
        # trained centroids: the assignment is the probe-1 list of every stored row, as the library's own probe gives it
        lid = f.list_ids()
        assert np.array_equal(lid, f.probe(rows, 1)[:, 0])
        with lib.Gallery.l2_from_host(cent) as gc:               # (an independent route to the same values: the exhaustive search)
            near, _, _, _, _ = gc.search_l2(rows, 1)
        assert np.array_equal(lid, near[:, 0])
        probes = f.probe(q, nprobe)
        ids, v64, _ = f.search(q, k, nprobe=nprobe, return_values64=True)
        for i in range(len(q)):
            w_ids, _, w64, _, _ = g.search_l2(q[i:i + 1], k, allow=np.isin(lid, probes[i]))
            assert np.array_equal(ids[i:i + 1], w_ids) and v64[i:i + 1].tobytes() == w64.tobytes()
        a_ids, a64, _ = f.search(q, k, nprobe=nlist, return_values64=True)
        w_ids, _, w64, _, _ = g.search_l2(q, k)
        assert np.array_equal(a_ids, w_ids) and a64.tobytes() == w64.tobytes()


def test_matcher_with_every_list_probed_is_the_exhaustive_matcher(lib, tmp_path, monkeypatch):
    from isehr_amd import nnsearch
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(15)
    train = rng.standard_normal((2000, 64)).astype(np.float32)
    train /= np.linalg.norm(train, axis=1, keepdims=True)
    test = rng.standard_normal((7, 64)).astype(np.float32)
    test /= np.linalg.norm(test, axis=1, keepdims=True)
    K, nlist = 10, 12
    idx, t = nnsearch.matching_IVF_hip(K, train, test, dataset="ivf_case", nlist=nlist, nprobe=nlist)
    want, _ = nnsearch.matching_L2_hip(K, train, test)
    assert idx.dtype == np.int64 and idx.shape == (7, K) and t > 0
    assert np.array_equal(idx, np.asarray(want))
    again, t2 = nnsearch.matching_IVF_hip(K, train, test, dataset="ivf_case", nlist=nlist, nprobe=nlist, ifgenerate=False)
    assert np.array_equal(again, idx) and t2 > 0
    few, _ = nnsearch.matching_IVF_hip(K, train, test, dataset="ivf_case", nlist=nlist, nprobe=2, ifgenerate=False)
    assert few.shape == (7, K) and (few >= 0).all()
    with pytest.raises(FileNotFoundError):
        nnsearch.matching_IVF_hip(K, train, test, dataset="ivf_case", nlist=nlist + 1, nprobe=2, ifgenerate=False)
