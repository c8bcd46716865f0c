"""GPU: k-means over whole rows at f64 matrix rate (csrc/kmeans.hip, csrc/api_kmeans.hip) against the numpy truth
of the PQ training with one book (tests/_pq_train_truth.py, restated for k > 256 in tests/_kmeans_truth.py) and against pqw_train in
the same process.  The contract is bit-exact: centroids are compared on their float32 bits, move counts, flagged counts and ids
with ==."""
import functools

import numpy as np
import pytest

from _kmeans_truth import assign_truth, flagged_cap, flagged_floor, lattice, near_ties, tau_rows, train_steps
from _pq_train_truth import clustered, default_init, train_truth

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
    return got[0].shape == want[0].shape and np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(got[1], want[1])


@functools.lru_cache(maxsize=None)
def _problem(n, k, d, iters=3, seed=0, shift=0.0):
    """clustered rows, the default initial rows and the truth from them: computed once, shared, read-only"""
    x, _ = clustered(np.random.RandomState(seed + n + 7 * k + 3 * d), n, 1, k, d)
    x = x + np.float32(shift)
    C0 = default_init(x, 1, k)[0]
    C, moved, caps = train_steps(x, k, iters, C0)
    if k <= 256:
        assert _same((C[None], moved), train_truth(x, 1, k, iters, C0[None]))      # the restated loop is the truth's
    ids = assign_truth(x, C)
    for a in (x, C0, C, moved, ids):
        a.setflags(write=False)
    return x, C0, C, moved, caps, ids


def _check_training(lib, x, k, iters, want_C, want_moved, caps, **kw):
    got = lib.kmeans_train(x, k, iters=iters, return_flagged=True, **kw)
    assert got[0].dtype == np.float32 and got[0].shape == want_C.shape and got[1].dtype == np.int64 and got[2].dtype == np.int64
    assert np.array_equal(got[1], want_moved), (got[1], want_moved)
    assert np.array_equal(_bits(got[0]), _bits(want_C))
    ran = len(caps)
    for t in range(ran):
        assert caps[t][0] <= got[2][t] <= caps[t][1], (t, got[2], caps)
    assert (got[2][ran:] == 0).all()
    return got


# ---- tile and chunk edges: n and k below, at and above the 128 x 128 tile and in a second row / column block, d below, at and above
# the K-chunk of 16 and over several chunks; k = 300 (three column blocks, ids beyond a byte) takes n = 300
NK = [(n, k) for n in (2, 127, 128, 129, 257) for k in (2, 127, 128, 129) if n >= k] + [(300, 300)]


@pytest.mark.parametrize("n,k", NK)
def test_training_and_assignment_at_tile_edges(lib, n, k):
    for d in (1, 15, 16, 17, 33, 64):
        x, C0, C, moved, caps, ids = _problem(n, k, d)
        _check_training(lib, x, k, 3, C, moved, caps)
        ref = lib.pqw_train(x, 1, k, iters=3)
        assert _same((C[None], moved), ref), (n, k, d)
        got_ids, flagged = lib.kmeans_assign(x, C, return_flagged=True)
        assert got_ids.dtype == np.int32 and np.array_equal(got_ids, ids), (n, k, d)
        assert flagged_floor(x, C) <= flagged <= flagged_cap(x, C), (n, k, d)


def test_training_over_2048_columns(lib):
    x, C0, C, moved, caps, ids = _problem(300, 130, 2048)
    _check_training(lib, x, 130, 3, C, moved, caps)
    assert _same((C[None], moved), lib.pqw_train(x, 1, 130, iters=3))
    assert np.array_equal(lib.kmeans_assign(x, C), ids)


# ---- the MFMA path must carry the result
@pytest.mark.parametrize("n,k,d", [(300, 130, 64), (257, 129, 17), (300, 130, 33), (129, 2, 1), (1000, 300, 2048)])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_matrix_kernel_decides_continuous_inputs(lib, n, k, d, seed):
    iters = 3 if d <= 64 else 2                                            # (the numpy truth of 2048 columns takes seconds)
    for shift in ((0.0, 100.0) if d <= 64 else (0.0,)):
        x, C0, C, moved, caps, ids = _problem(n, k, d, iters=iters, seed=seed, shift=shift)
        assert all(hi <= n // 100 for _, hi in caps), caps                # the truth itself stays within the cap
        got = _check_training(lib, x, k, iters, C, moved, caps)
        assert (got[2] <= n // 100).all(), got[2]
        got_ids, flagged = lib.kmeans_assign(x, C, return_flagged=True)
        assert np.array_equal(got_ids, ids) and flagged <= n // 100


# ---- the fallback must carry the result
def test_duplicated_centroids_go_to_the_lower_id(lib):
    """(a): every centroid twice, once next to itself and once a column block away: every row ties, the direct form decides all"""
    x, C0, _, _, _, _ = _problem(300, 130, 33)
    n = x.shape[0]
    for init in (np.repeat(C0[:80], 2, axis=0), np.concatenate([C0, C0])):
        k = init.shape[0]
        C, moved, caps = train_steps(x, k, 3, init)
        assert caps[0] == (n, n)
        got = _check_training(lib, x, k, 3, C, moved, caps, init=init)
        assert got[2][0] == n
        assert _same((C[None], moved), lib.pqw_train(x, 1, k, iters=3, init=init[None]))
        ids, flagged = lib.kmeans_assign(x, init, return_flagged=True)
        want = assign_truth(x, init)
        assert np.array_equal(ids, want) and flagged == n
        assert (want % 2 == 0).all() if k == 160 else (want < 130).all()


def test_lattice_rows_with_exact_ties(lib):
    """(b): coordinates in {-2 .. 2}, d = 17: exact ties between distinct centroids, also across column blocks"""
    x, C0 = lattice(np.random.RandomState(3), 400, 150)
    want = assign_truth(x, C0)
    ids, flagged = lib.kmeans_assign(x, C0, return_flagged=True)
    assert np.array_equal(ids, want)
    assert flagged >= flagged_floor(x, C0) >= 40
    C, moved, caps = train_steps(x, 150, 3, C0)
    _check_training(lib, x, 150, 3, C, moved, caps, init=C0)
    assert _same((C[None], moved), lib.pqw_train(x, 1, 150, iters=3, init=C0[None]))


def test_rows_whose_bound_exceeds_every_gap(lib):
    """(c): float64 rows offset by 1e6 with unit spread: tau (7.5e3 at d = 2048) exceeds every gap (the squared distances are
    about 2 d +- 130), every row goes to the direct form.  The initial centroids are not rows: a row is 4e3 nearer to itself"""
    rng = np.random.RandomState(4)
    n, k, d = 200, 8, 2048
    x = 1e6 + rng.randn(n, d)
    C0 = (1e6 + 0.5 * rng.randn(k, d)).astype(np.float32)
    C, moved, caps = train_steps(x, k, 3, C0)
    assert all(c == (n, n) for c in caps), (caps, tau_rows(x, C0).min())
    got = _check_training(lib, x, k, 3, C, moved, caps, init=C0)
    assert (got[2][:len(caps)] == n).all()
    assert _same((C[None], moved), lib.pqw_train(x, 1, k, iters=3, init=C0[None]))
    ids, flagged = lib.kmeans_assign(x, C, return_flagged=True)
    assert np.array_equal(ids, assign_truth(x, C)) and flagged == n


def test_near_ties_across_the_bound(lib):
    x, C = near_ties()
    want = assign_truth(x, C)
    ids, flagged = lib.kmeans_assign(x, C, return_flagged=True)
    assert np.array_equal(ids, want), (ids, want)
    assert flagged_floor(x, C) <= flagged <= flagged_cap(x, C)
    assert 4 <= flagged <= 8                                   # s = 0 and 1e-3 must be flagged, s = 1e3 must not


# ---- layouts and types
def test_layouts_and_types_give_the_packed_answer(lib):
    x, C0, C, moved, caps, ids = _problem(257, 129, 33)
    n, d = x.shape
    x64 = x.astype(np.float64)
    wide = np.full((n, d + 5), np.float32(7e3))
    wide[:, :d] = x
    views = {"float64": x64, "[D, N]": np.ascontiguousarray(x.T).T, "[D, N] float64": np.ascontiguousarray(x64.T).T,
             "row-strided": wide[:, :d], "every other row": np.repeat(x, 2, axis=0)[::2]}
    assert views["[D, N]"].strides == (4, 4 * n) and views["row-strided"].strides[0] == 4 * (d + 5)
    for name, v in views.items():
        assert _same(lib.kmeans_train(v, 129, iters=3), (C, moved)), name
        assert np.array_equal(lib.kmeans_assign(v, C), ids), name


@pytest.mark.parametrize("k", [1000, 1024])
def test_eight_column_blocks_take_the_xcd_tile_order(lib, k):
    """k = 1000 and 1024: 8 column blocks (the last ragged at 1000), so km_assign_mfma_kernel decodes its tile by the XCD-aware
    branch of f64t_tile_order (csrc/f64_tile_order.h); n = 130, d = 33: two row tiles, ragged rows and K.  Lattice rows and
    centroids (coordinates in {-2 .. 2}): every sum of either form is an integer below 2^53, exact in any order, so the ids are
    the float64 direct-form argmin whatever the tile a centroid was scored in.  Contiguous float32, [D, N] and float64 rows,
    typed and device forms."""
    import torch
    n, d = 130, 33
    x, C = lattice(np.random.RandomState(11 + k), n, k, d=d)
    for a in (x, C):                                           # the precondition: small integers, so every partial sum is exact
        assert np.array_equal(a, np.rint(a)) and np.abs(a).max() <= 2
    assert d * (2 + 2) ** 2 < 2 ** 53
    want = assign_truth(x, C)
    assert len(np.unique(want // 128)) == 8                    # every column block wins somewhere: a misplaced tile shows
    x64 = x.astype(np.float64)
    views = {"float32": x, "[D, N]": np.ascontiguousarray(x.T).T, "float64": x64}
    assert views["[D, N]"].strides == (4, 4 * n)
    cd = torch.from_numpy(np.array(C)).cuda()
    bytes_ = lib.kmeans_assign_workspace_bytes(k, n)
    for name, v in views.items():
        assert np.array_equal(lib.kmeans_assign(v, C), want), name
        t = torch.from_numpy(np.ascontiguousarray(v.T)).cuda().t() if name == "[D, N]" else torch.from_numpy(np.array(v)).cuda()
        assert tuple(t.stride()) == tuple(s // v.itemsize for s in v.strides)
        out = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        ws = torch.empty(bytes_, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        lib.kmeans_assign_device(t.data_ptr(), n, d, cd.data_ptr(), k, out.data_ptr(), ws.data_ptr(), bytes_,
                                 dtype=lib.MI_F32 if t.dtype == torch.float32 else lib.MI_F64, row_stride=t.stride(0),
                                 col_stride=t.stride(1), stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), want), name


def test_the_layout_sweep_of_the_typed_entry_points(lib):
    """every view of tests/_layouts.py (contiguous, [D, N], padded rows, every other column, a sub-block; float32 and float64),
    embedded in buffers whose other elements are NaN, through the three typed entry points: the answer is the contiguous float32
    one, byte for byte, so nothing outside the view was read.  The float64 views hold values float32 cannot (planted elements):
    an entry point that rounded its rows to float32 would give the float32 answer there, which is checked to differ."""
    import torch
    import _layouts as L
    x, C0, C, moved, caps, ids = _problem(257, 129, 33)
    x = np.ascontiguousarray(x)
    n, d = x.shape
    k = 129
    cd = torch.from_numpy(np.array(C)).cuda()
    bytes_ = lib.kmeans_assign_workspace_bytes(k, n)
    seen = []
    for lay in L.layouts(x, np.nan):
        seen.append(lay.name)
        assert _same(lib.kmeans_train(lay.view, k, iters=3), (C, moved)), lay.name
        assert np.array_equal(lib.kmeans_assign(lay.view, C), ids), lay.name
        t = L.on_device(lay)
        rs, cs = L.element_strides(lay.view)
        out = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        ws = torch.empty(bytes_, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        lib.kmeans_assign_device(t.data_ptr(), n, d, cd.data_ptr(), k, out.data_ptr(), ws.data_ptr(), bytes_,
                                 dtype=lib.MI_F32 if t.dtype == torch.float32 else lib.MI_F64, row_stride=rs, col_stride=cs,
                                 stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), ids), lay.name
        got = lib.kmeans_train_device(t.data_ptr(), n, d, k, 3, dtype=lib.MI_F32 if t.dtype == torch.float32 else lib.MI_F64,
                                      row_stride=rs, col_stride=cs)
        assert _same(got, (C, moved)), lay.name
    assert seen == ["c32", "c64", "t32", "t64", "pad32", "pad64", "col32", "col64", "sub32"]
    # float64 rows are read as float64: between centroids at 0 and 2 a row at 1 +- 2^-40 has a side, its float32 rounding (1) ties
    c2 = np.zeros((2, d), np.float32)
    c2[1, 0] = 2.0
    mid = np.zeros((2, d), np.float64)
    mid[:, 0] = [1.0 + 2.0 ** -40, 1.0 - 2.0 ** -40]
    for lay in L.layouts(mid.astype(np.float32), np.nan):
        if lay.name.endswith("64"):
            lay.view[...] = mid
            assert np.array_equal(lib.kmeans_assign(lay.view, c2), [1, 0]), lay.name
            t = L.on_device(lay)
            rs, cs = L.element_strides(lay.view)
            out = torch.full((2,), -7, dtype=torch.int32, device="cuda")
            ws = torch.empty(lib.kmeans_assign_workspace_bytes(2, 2), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            lib.kmeans_assign_device(t.data_ptr(), 2, d, torch.from_numpy(c2).cuda().data_ptr(), 2, out.data_ptr(), ws.data_ptr(),
                                     ws.numel(), dtype=lib.MI_F64, row_stride=rs, col_stride=cs)
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy(), [1, 0]), lay.name
    assert np.array_equal(lib.kmeans_assign(mid.astype(np.float32), c2), [0, 0])


def test_host_rows_pass_in_several_blocks(lib):
    """2100 float64 rows of 4096 columns are more than one 64 MiB block of the host form"""
    rng = np.random.RandomState(6)
    C = (rng.randn(3, 4096) * 2).astype(np.float32)
    x = C[rng.randint(0, 3, 2100)].astype(np.float64) + 0.5 * rng.randn(2100, 4096)
    ids, flagged = lib.kmeans_assign(x, C, return_flagged=True)
    assert np.array_equal(ids, assign_truth(x, C)) and flagged == 0


# ---- resume and early stop
def test_resume_is_bit_exact(lib):
    x, C0, _, _, _, _ = _problem(257, 129, 17)
    full = lib.kmeans_train(x, 129, iters=5)
    first = lib.kmeans_train(x, 129, iters=2)
    second = lib.kmeans_train(x, 129, iters=3, init=first[0])
    assert np.array_equal(_bits(second[0]), _bits(full[0]))
    assert np.array_equal(first[1], full[1][:2]) and np.array_equal(second[1][1:], full[1][3:])
    assert _same(full, tuple(a[0] if a.ndim == 3 else a for a in lib.pqw_train(x, 1, 129, iters=5)))


def test_early_stop_leaves_zeros(lib):
    rng = np.random.RandomState(8)
    cent = np.eye(5, 20, dtype=np.float32) * 100
    x = (cent[np.arange(300) % 5] + 0.1 * rng.randn(300, 20)).astype(np.float32)
    C, moved, caps = train_steps(x, 5, 8, default_init(x, 1, 5)[0])
    assert len(caps) < 8 and moved[len(caps) - 1] == 0
    got = _check_training(lib, x, 5, 8, C, moved, caps)
    assert (got[1][len(caps):] == 0).all() and (got[2] == 0).all()
    a, u = lib.pq_train_timing()                               # the timing entry point reports this call too
    assert len(a) == len(caps) and len(u) == len(caps) - 1


# ---- device form
@pytest.mark.parametrize("case", ["unflagged", "flagged"])
def test_device_form_on_a_side_stream(lib, case):
    import torch
    x, C0, C, _, _, _ = _problem(300, 130, 33)
    cent = C if case == "unflagged" else np.concatenate([C, C])
    k, (n, d) = cent.shape[0], x.shape
    want, want_flagged = lib.kmeans_assign(x, cent, return_flagged=True)
    assert want_flagged == (0 if case == "unflagged" else n)
    xd = torch.from_numpy(np.array(x)).cuda()
    xt = torch.from_numpy(np.ascontiguousarray(x.T)).cuda()                    # the [D, N] layout on the device
    cd = torch.from_numpy(np.array(cent)).cuda()
    # the largest chunks and the smallest (128 rows: three chunks, the last one partial)
    for bytes_ in (lib.kmeans_assign_workspace_bytes(k, n), lib.kmeans_assign_workspace_bytes(k, 128)):
        for rows, rs, cs in ((xd, d, 1), (xt, 1, n)):
            ws = torch.empty(bytes_, dtype=torch.uint8, device="cuda")
            out = torch.full((n + 2,), -7, dtype=torch.int32, device="cuda")
            fl = torch.full((1,), 99, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            side = torch.cuda.Stream()
            with torch.cuda.stream(side):
                lib.kmeans_assign_device(rows.data_ptr(), n, d, cd.data_ptr(), k, out.data_ptr(), ws.data_ptr(), bytes_,
                                         flagged_ptr=fl.data_ptr(), row_stride=rs, col_stride=cs, stream=side.cuda_stream)
            side.synchronize()
            o = out.cpu().numpy()
            assert np.array_equal(o[:n], want) and (o[n:] == -7).all()
            assert int(fl.cpu()[0]) == want_flagged
    with pytest.raises(RuntimeError):
        lib.kmeans_assign_device(xd.data_ptr(), n, d, cd.data_ptr(), k, out.data_ptr(), ws.data_ptr(), 64)      # no room for 128 rows


# ---- Python surface
def test_kmeans_class_and_ivfflat_train_matrix(lib):
    x, _, _, _, _, _ = _problem(300, 130, 33)
    km = lib.KMeans(130, iters=4, seed=3).fit(x)
    want = lib.kmeans_train(x, 130, iters=4, seed=3)
    assert np.array_equal(_bits(km.cluster_centers_), _bits(want[0])) and km.cluster_centers_.shape == (130, 33)
    assert np.array_equal(km.labels_, lib.kmeans_assign(x, km.cluster_centers_)) and km.labels_.dtype == np.int32
    assert 1 <= km.n_iter_ <= 4
    new = (x[:50] + np.float32(0.25)).astype(np.float64)
    assert np.array_equal(km.predict(new), assign_truth(new, km.cluster_centers_))
    a = lib.IVFFlatIndex.train_matrix(x, 130)
    b = lib.IVFFlatIndex.train(x, 130)
    assert a.shape == b.shape == (130, 33) and a.dtype == b.dtype == np.float32 and np.array_equal(_bits(a), _bits(b))
    a = lib.IVFFlatIndex.train_matrix(x, 130, iters=3, seed=5)
    assert np.array_equal(_bits(a), _bits(lib.IVFFlatIndex.train(x, 130, iters=3, seed=5)))
