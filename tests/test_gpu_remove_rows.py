"""GPU: rows removed from a gallery in place (mi_gallery_remove_rows, Gallery.remove, KNN.remove_ids).

The contract: after the call every section of the prepared gallery equals, bit for bit, what the same ingest path writes for the
surviving source rows alone at the same image type.  So each case saves the gallery, holds the file to the float64 reference of
tests/_gallery_file.py, and compares it section by section with the file of a gallery built fresh from X[kept].  Shapes are the
smallest that reach every hazard of the in-place move: n = 1500 is six tiles of 256 rows with the last one partial, d = 96 gives
dp = 128 with padding columns, and "remove_block_rows" = 256 makes the move cross several staging blocks."""
import functools
import os

import numpy as np
import pytest

import _gallery_file as gfile

pytestmark = pytest.mark.gpu

N, CAP = 1500, 2048
PATTERNS = ["row0", "last", "tile1", "rows1_255", "every2nd", "rand1pct", "rand90pct", "tail256", "all_but_777", "all", "none"]


def _mask(pattern, n=N):
    m = np.zeros(n, bool)
    if pattern == "row0":
        m[0] = True
    elif pattern == "last":
        m[n - 1] = True
    elif pattern == "tile1":
        m[256:512] = True
    elif pattern == "rows1_255":
        m[1:256] = True
    elif pattern == "every2nd":
        m[::2] = True
    elif pattern == "rand1pct":
        m[np.random.default_rng(11).choice(n, n // 100, replace=False)] = True
    elif pattern == "rand90pct":
        m[np.random.default_rng(12).choice(n, n * 9 // 10, replace=False)] = True
    elif pattern == "tail256":
        m[n - 256:] = True
    elif pattern == "all_but_777":
        m[:] = True
        m[777] = False
    elif pattern == "all":
        m[:] = True
    else:
        assert pattern == "none"
    return m


@functools.lru_cache(maxsize=None)
def _rows(d, norm, large=True):
    x = np.random.default_rng(1000 + d).standard_normal((N + 300, d), dtype=np.float32)
    if norm == gfile.NORM_NONE:
        x *= np.float32(0.5 / np.sqrt(d))                      # raw rows of norm ~0.5, inside fp16's comfortable range ...
        if large:
            x[700] *= np.float32(30.0 / np.linalg.norm(x[700].astype(np.float64)))  # ... but for one row of norm 30
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _ref(d, norm, large=True):
    return gfile.reference_rows(_rows(d, norm, large), norm)


def _build(kind, x, d, norm):
    """The three constructors: from_host (fp16 unless raw rows are large), the same re-imaged to bf16, appendable (two appends)."""
    from isehr_amd import _lib
    if kind == "appendable":
        g = _lib.Gallery.empty(CAP, d, norm_mode=norm)
        if len(x):
            h = len(x) // 2
            for part in (x[:h], x[h:]):
                if len(part):
                    g.append(part)
        return g
    g = _lib.Gallery.from_host(x, norm_mode=norm)
    if kind == "bf16":
        g.set_image_dtype(0)
    return g


def _file(g, path):
    g.save(path)
    f = gfile.read_gallery_file(path)
    os.unlink(path)
    return f


def _same_sections(a, b, what):
    assert (a.n, a.npad, a.d, a.dp, a.norm_mode, a.img_f16) == (b.n, b.npad, b.d, b.dp, b.norm_mode, b.img_f16), what
    for name in ("rows_f32", "rowstat", "gstat3"):
        x, y = np.ascontiguousarray(getattr(a, name)).view(np.uint32), np.ascontiguousarray(getattr(b, name)).view(np.uint32)
        assert np.array_equal(x, y), "%s: %s differs (%d words, first %s)" % (what, name, int((x != y).sum()),
                                                                          np.argwhere(x != y)[:3].tolist())
    assert np.array_equal(a.image_bits, b.image_bits), "%s: image differs at (row, col) %s" % (
        what, np.argwhere(a.image_bits != b.image_bits)[:3].tolist())


def _remove_case(tmp_path, pattern, kind, d, norm, block, large=True):
    from isehr_amd import _lib
    X, ref = _rows(d, norm, large), _ref(d, norm, large)
    extra = X[N:]
    mask = _mask(pattern)
    path = str(tmp_path / "g.bin")
    _lib.set_global_option("remove_block_rows", block)
    g = fresh = None
    try:
        g = _build(kind, X[:N], d, norm)
        f16 = int(g.get_option("image_dtype"))
        before = _file(g, path) if pattern == "none" else None
        kept = g.remove(mask)
        assert np.array_equal(kept, np.flatnonzero(~mask)) and g.n == kept.size
        assert int(g.get_option("image_dtype")) == f16, "the image type changed"
        if pattern == "none":
            _same_sections(_file(g, path), before, "no rows removed")
            return
        if kept.size == 0:
            # nothing to save: an append on the emptied gallery must equal the same append on an empty one
            g.append(extra)
            fresh = _lib.Gallery.empty(CAP, d, norm_mode=norm)
            fresh.set_image_dtype(f16)
            fresh.append(extra)
            got = _file(g, path)
            gfile.check_all(got, ref=ref[N:], get_rows=g.get_rows(0, 300), norm_bounds=g.norm_bounds())
            _same_sections(got, _file(fresh, path), "append after removing every row")
            return
        got = _file(g, path)
        assert (got.n, got.npad, got.img_f16) == (kept.size, -(-kept.size // 256) * 256, f16)
        gfile.check_all(got, ref=ref[kept], get_rows=g.get_rows(0, kept.size), norm_bounds=g.norm_bounds())
        fresh = _build(kind, X[kept], d, norm)
        fresh.set_image_dtype(f16)
        _same_sections(got, _file(fresh, path), "removed vs fresh")
        if kind == "appendable":
            # rows n' .. old npad were zeroed: appends write their own rows only, so the next append shows what was left there
            g.append(extra)
            fresh.append(extra)
            _same_sections(_file(g, path), _file(fresh, path), "append after the removal")
    finally:
        _lib.set_global_option("remove_block_rows", 0)
        for h in (g, fresh):
            if h is not None:
                h.close()


@pytest.mark.parametrize("block", [256, 0])
@pytest.mark.parametrize("d", [96, 2048])
@pytest.mark.parametrize("kind", ["fp16", "bf16", "appendable"])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_every_section_equals_a_fresh_ingest_of_the_survivors(tmp_path, pattern, kind, d, block):
    _remove_case(tmp_path, pattern, kind, d, gfile.NORM_L2, block)


# "none": raw rows with one row of norm 30 -- from_host stores such a gallery as bf16 by itself, so its "fp16" and "bf16" kinds
# are one case (the second is left out); "none_small": raw rows without it, a raw fp16 gallery
NORMS = {"l2eps": (gfile.NORM_L2_EPS, True), "none": (gfile.NORM_NONE, True), "none_small": (gfile.NORM_NONE, False)}


NORM_KINDS = [(nm, kd) for nm in NORMS for kd in ("fp16", "bf16", "appendable") if (nm, kd) != ("none", "bf16")]


@pytest.mark.parametrize("block", [256, 0])
@pytest.mark.parametrize("d", [96, 2048])
@pytest.mark.parametrize("norm,kind", NORM_KINDS)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_other_norm_modes(tmp_path, pattern, norm, kind, d, block):
    mode, large = NORMS[norm]
    _remove_case(tmp_path, pattern, kind, d, mode, block, large)


def test_the_raw_gallery_without_a_large_row_is_fp16():
    """What makes the "none_small" cases above the raw fp16 ones."""
    from isehr_amd import _lib
    for d in (96, 2048):
        g = _lib.Gallery.from_host(_rows(d, gfile.NORM_NONE, False)[:N], norm_mode=gfile.NORM_NONE)
        try:
            assert int(g.get_option("image_dtype")) == 1 and g.norm_bounds()[0] < 4.0
        finally:
            g.close()


def test_raw_gallery_maxima_fall_and_the_image_type_stays(tmp_path):
    """NORM_NONE with one row of norm 30: the gallery is bf16 because of that row.  Removing it leaves the maxima of the others
    (check_maxima demands the maximum over the rows < n, not over a superset) and leaves the image type alone."""
    from isehr_amd import _lib
    X = _rows(96, gfile.NORM_NONE)[:N]
    g = _lib.Gallery.from_host(X, norm_mode=gfile.NORM_NONE)
    fresh = None
    try:
        assert int(g.get_option("image_dtype")) == 0 and g.norm_bounds()[0] > 29.0
        kept = g.remove([700])
        assert int(g.get_option("image_dtype")) == 0
        assert g.norm_bounds()[0] < 4.0
        got = _file(g, str(tmp_path / "g.bin"))
        gfile.check_all(got, ref=_ref(96, gfile.NORM_NONE)[kept], get_rows=g.get_rows(0, g.n), norm_bounds=g.norm_bounds())
        fresh = _lib.Gallery.from_host(X[kept], norm_mode=gfile.NORM_NONE)
        assert int(fresh.get_option("image_dtype")) == 1         # built anew the same rows would be fp16 ...
        fresh.set_image_dtype(0)                                 # ... which is the caller's decision, not the removal's
        _same_sections(got, _file(fresh, str(tmp_path / "f.bin")), "removed vs fresh")
    finally:
        g.close()
        if fresh is not None:
            fresh.close()


# ---- the answers ------------------------------------------------------------------------------------------------------------
def _bits_equal(a, b):
    assert np.array_equal(a[0], b[0])
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def _answers_data():
    rng = np.random.default_rng(77)
    n, d, nq = 5000, 128, 37
    X = rng.standard_normal((n, d), dtype=np.float32)
    src = rng.choice(n, 40, replace=False)
    dst = rng.choice(np.setdiff1d(np.arange(n), src), 40, replace=False)
    X[dst[:20]] = X[src[:20]]                                                # exact ties
    X[dst[20:]] = X[src[20:]] * np.float32(1 + 1e-6)                         # near-ties
    Q = np.concatenate([X[src[:30]] + np.float32(0.01) * rng.standard_normal((30, d), dtype=np.float32),
                        rng.standard_normal((nq - 30, d), dtype=np.float32)])
    return X, Q


@pytest.mark.parametrize("row_offset", [0, 2 ** 33])
def test_answers_equal_a_fresh_gallery_of_the_survivors(row_offset):
    from isehr_amd import _lib
    X, Q = _answers_data()
    n, k = len(X), 100
    g = _lib.Gallery.from_host(X, row_offset=row_offset)
    fresh = None
    try:
        top, _, _ = g.search(Q, k)
        assert top.min() >= row_offset
        mask = np.random.default_rng(78).random(n) < 0.3
        mask[(top[:, [0, 3, 7]] - row_offset).ravel()] = True               # some of every query's current top-10
        kept = g.remove(np.flatnonzero(mask) + row_offset)                   # global ids
        assert np.array_equal(kept, np.flatnonzero(~mask) + row_offset) and g.n == kept.size
        fresh = _lib.Gallery.from_host(X[kept - row_offset], row_offset=row_offset)
        got, want = g.search(Q, k), fresh.search(Q, k)
        _bits_equal(got, want)
        assert got[0].min() >= row_offset and got[0].max() < row_offset + g.n
        assert np.array_equal(got[0], g.dense64_search(Q, k)[0])
        # the rows behind the returned ids are the survivors' (kept maps new ids to old ones)
        assert np.array_equal(g.get_rows(0, g.n).view(np.uint32), fresh.get_rows(0, g.n).view(np.uint32))
        tau = float(np.sort(got[1], axis=1)[:, k // 2].mean())
        r1, r2 = g.range_search(Q, tau), fresh.range_search(Q, tau)
        assert np.array_equal(r1[0], r2[0]) and r1[0][-1] > 0
        _bits_equal(r1[1:3], r2[1:3])
        d64 = g.dense64_search(Q, 2048)
        for i in range(len(Q)):                                              # the hits are dense64's rows at or above tau
            cnt = int(r1[0][i + 1] - r1[0][i])
            assert cnt < 2048 and np.array_equal(r1[1][r1[0][i]:r1[0][i + 1]], d64[0][i, :cnt])
        p1, p2 = g.rank_prefix(Q, 300, return_scores=True), fresh.rank_prefix(Q, 300, return_scores=True)
        _bits_equal(p1[:2], p2[:2])
        allow = np.random.default_rng(79).random(g.n) < 0.5
        d64a = np.stack([row[allow[row - row_offset]][:k] for row in d64[0]])
        for path in (1, 2):
            for h in (g, fresh):
                h.set_option("filter_path", path)
            f1, f2 = g.search_filtered(Q, k, allow), fresh.search_filtered(Q, k, allow)
            _bits_equal(f1[:2], f2[:2])
            assert f1[3]["path"] == path and np.array_equal(f1[0], d64a)
    finally:
        g.close()
        if fresh is not None:
            fresh.close()


# ---- squared L2 ---------------------------------------------------------------------------------------------------------------
def test_l2_gallery_and_knn_remove_ids():
    from isehr_amd import _lib
    from isehr_amd.knn import KNN
    rng = np.random.default_rng(90)
    n, d, k = 1500, 96, 50
    X = rng.standard_normal((n, d), dtype=np.float32)
    X *= (np.float32(30.0) / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)
    Q = X[rng.choice(n, 20, replace=False)] + rng.standard_normal((20, d), dtype=np.float32)
    ids = np.arange(0, n, 3)
    g = _lib.Gallery.l2_from_host(X)
    fresh = knn = None
    try:
        kept = g.remove(ids)
        assert np.array_equal(kept, np.setdiff1d(np.arange(n), ids)) and g.n == n - len(ids) and g.d == d
        assert np.array_equal(g.get_rows(0, g.n).view(np.uint32), X[kept].view(np.uint32))     # (the hidden columns: tests/test_gpu_l2_gallery_reference.py)
        fresh = _lib.Gallery.l2_from_host(X[kept])
        a, b, c = g.search_l2(Q, k), fresh.search_l2(Q, k), g.dense64_search_l2(Q, k)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[2].view(np.uint64), b[2].view(np.uint64))
        assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
        # the dense checker sums the same d exact squares in another order: ids equal, each float64 distance within
        # 2 d u of the other (u = 2^-53; either sum is within d u, relative, of the exact one) -- the bound tests/test_gpu_l2_search.py
        # holds the two paths to; against the fresh gallery (the same path) the bits are equal, above
        assert np.array_equal(a[0], c[0])
        assert np.abs(a[2] - c[2]).max() <= 2.0 * d * 2.0 ** -53 * c[2].max()
        knn = KNN(X, "euclidean")
        assert knn.remove_ids(ids) == len(ids) and knn.N == g.n
        dist, idx = knn.search(Q, k)
        assert np.array_equal(idx, a[0]) and np.array_equal(dist.view(np.uint32), a[1].view(np.uint32))
    finally:
        g.close()
        for h in (fresh, knn):
            if h is not None:
                h.close()


def test_knn_cosine_remove_ids():
    from isehr_amd.knn import KNN
    X, Q = _answers_data()
    ids = np.arange(5, len(X), 7)
    a, b = KNN(X), KNN(np.delete(X, ids, axis=0))
    try:
        assert a.remove_ids(ids) == len(ids) and a.N == b.N
        (s1, i1), (s2, i2) = a.search(Q, 20), b.search(Q, 20)
        assert np.array_equal(i1, i2) and np.array_equal(s1.view(np.uint32), s2.view(np.uint32))
    finally:
        a.close()
        b.close()


# ---- state that would go stale --------------------------------------------------------------------------------------------------
def test_filtered_search_cache_is_dropped():
    """A remove followed by an append of as many rows restores n: the cached sub-gallery's key (bitmap, n) would match again."""
    from isehr_amd import _lib
    rng = np.random.default_rng(31)
    n, d, k = 3000, 128, 20
    X = rng.standard_normal((n + 64, d), dtype=np.float32)
    Q = rng.standard_normal((9, d), dtype=np.float32)
    W = rng.random(n) < 0.05
    g = _lib.Gallery.empty(4096, d)
    fresh = None
    try:
        g.append(X[:n])
        g.set_option("filter_cache", 1)
        g.set_option("filter_path", 1)
        g.search_filtered(Q, k, W)
        assert g.search_filtered(Q, k, W)[3]["cache_hit"] == 1             # the sub-gallery is cached
        gone = np.flatnonzero(W)[:64]                                       # allowed rows leave: their slots get other rows
        kept = g.remove(gone)
        g.append(X[n:])
        assert g.n == n
        got = g.search_filtered(Q, k, W)
        assert got[3]["cache_hit"] == 0
        fresh = _lib.Gallery.from_host(np.concatenate([X[kept], X[n:]]))
        fresh.set_option("filter_path", 1)
        _bits_equal(got[:2], fresh.search_filtered(Q, k, W)[:2])
    finally:
        g.close()
        if fresh is not None:
            fresh.close()


def test_diffusion_state_is_dropped():
    from isehr_amd import _lib
    rng = np.random.default_rng(32)
    X = rng.standard_normal((600, 32), dtype=np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    Q = X[:4].copy()
    never = _lib.Gallery.from_host(X[1:], norm_mode=_lib.NORM_NONE)
    g = _lib.Gallery.from_host(X, norm_mode=_lib.NORM_NONE)
    try:
        with pytest.raises(RuntimeError) as want:
            never.diffusion_online(Q, 3, 3, 100)
        g.diffusion_offline(100, 20)
        g.diffusion_online(Q, 3, 3, 100)                                     # answers while the offline matrix is there
        g.remove([0])
        with pytest.raises(RuntimeError) as got:
            g.diffusion_online(Q, 3, 3, 100)
        assert str(got.value) == str(want.value)
        g.diffusion_offline(100, 20)                                         # and the handle takes a new one
        g.diffusion_online(Q, 3, 3, 100)
    finally:
        g.close()
        never.close()


def test_pending_deferred_tail_completes_in_the_old_numbering():
    import torch
    from isehr_amd import _lib
    rng = np.random.default_rng(33)
    n, d, k, nq = 20000, 128, 50, 512
    X = rng.standard_normal((n, d), dtype=np.float32)
    Q = rng.standard_normal((nq, d), dtype=np.float32)
    g = _lib.Gallery.from_host(X)
    fresh = None
    try:
        want_old = g.search(Q, k)[0]
        q = torch.from_numpy(Q).cuda()
        ix = torch.full((nq, k), -5, dtype=torch.int64, device="cuda")
        mask = rng.random(n) < 0.2
        mask[want_old[:, 0]] = True
        g.set_option("async_tail", 3)
        try:
            torch.cuda.synchronize()
            g.search_device(q.data_ptr(), nq, k, ix.data_ptr())             # its tail is deferred to the next call
            kept = g.remove(mask)
            g.join()
            torch.cuda.synchronize()
        finally:
            g.set_option("async_tail", 0)
        assert np.array_equal(ix.cpu().numpy(), want_old)                   # answered before any row moved
        assert g.flags() == 0
        fresh = _lib.Gallery.from_host(X[kept])
        _bits_equal(g.search(Q, k)[:2], fresh.search(Q, k)[:2])
        # the same through the host entry point with several internal batches ("stream_tail")
        big = np.ascontiguousarray(np.tile(Q, (5, 1)))
        assert g.get_option("stream_tail") == 1
        _bits_equal(g.search(big, k)[:2], fresh.search(big, k)[:2])
    finally:
        g.close()
        if fresh is not None:
            fresh.close()


def test_refused_under_a_live_online_handle(tmp_path):
    from isehr_amd import _lib
    rng = np.random.default_rng(34)
    X = rng.standard_normal((2000, 64), dtype=np.float32)
    g = _lib.Gallery.from_host(X)
    never = _lib.Gallery.from_host(X)
    chain = _lib.OnlineChain(g, None, 10, max_batch=8, max_wait_us=100)
    try:
        before = _file(g, str(tmp_path / "a.bin"))
        with pytest.raises(RuntimeError, match="online handle"):
            g.remove([1, 2, 3])
        assert g.n == 2000
        _same_sections(_file(g, str(tmp_path / "b.bin")), before, "refused removal")
        want = never.search(X[:3], 10)[0]
        assert np.array_equal(chain.query(np.ascontiguousarray(X[:3]).ctypes.data, 3, _lib.MI_HOST), want)
    finally:
        chain.close()
        assert g.remove([1, 2, 3]).size == 1997                             # allowed again once the chain is gone
        g.close()
        never.close()


def test_device_bitmap_and_out_removed():
    import ctypes as C
    import torch
    from isehr_amd import _lib
    X = _rows(96, gfile.NORM_L2)[:N]
    mask = _mask("every2nd")
    bits = _lib.allow_bitmap(mask, N)
    junk = bits.copy()
    junk[-1] |= np.uint64(0xFFFF) << np.uint64(48)                           # bits at or beyond n are ignored
    dev = torch.from_numpy(junk.view(np.int64)).cuda()
    torch.cuda.synchronize()
    g, h = _lib.Gallery.from_host(X), _lib.Gallery.from_host(X)
    try:
        removed = C.c_int64(-1)
        _lib.check(_lib.load().mi_gallery_remove_rows(g._h, C.c_void_p(dev.data_ptr()), _lib.MI_DEVICE, C.byref(removed)))
        assert removed.value == int(mask.sum())
        kept = h.remove(mask)
        n2 = C.c_int64()
        _lib.check(_lib.load().mi_gallery_info(g._h, n2, None, None, None, None, None))
        assert n2.value == kept.size
        assert np.array_equal(g.get_rows(0, kept.size).view(np.uint32), h.get_rows(0, kept.size).view(np.uint32))
    finally:
        g.close()
        h.close()


# ---- the memory bound -----------------------------------------------------------------------------------------------------------
def test_extra_device_memory_is_bounded_by_the_staging_block():
    """n = 200 000, D = 2048, remove_block_rows = 4096: device memory may grow by the staging area (B rows of f32, image and
    RowStat), the keep-list (4 B per row), the bitmap and the scan buffers -- not by a second copy of the shard (2.4 GB here)."""
    import torch
    from isehr_amd import _lib
    n, d, B = 200_000, 2048, 4096
    X = np.random.default_rng(35).standard_normal((n, d), dtype=np.float32)
    Q = X[:8] + np.float32(0.1)
    g = _lib.Gallery.from_host(X)
    _lib.set_global_option("remove_block_rows", B)
    try:
        g.search(Q, 10)                                      # the handle has searched once: workspace, sample
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        mask = np.zeros(n, bool)
        mask[9::10] = True
        kept = g.remove(mask)
        torch.cuda.synchronize()
        grown = free0 - torch.cuda.mem_get_info()[0]
        bound = B * (d * 6 + 12) + 4 * n + n // 8 + (1 << 20)
        print("device memory grown by %.2f MiB, bound %.2f MiB" % (grown / 2 ** 20, bound / 2 ** 20))
        assert grown < bound
        assert g.n == n - 20000
        got = g.search(Q, 10)[0]
        assert np.array_equal(kept[got[:, 0]], np.arange(8))                 # rows 0..7 survive (9::10 spares them) and rank first
        sample = np.array([0, 1, 4095, 4096, 100_000, g.n - 1])
        for j in sample:
            want = X[kept[j]].astype(np.float64)
            want = (want / np.sqrt((want * want).sum())).astype(np.float32)
            assert np.abs(g.get_rows(int(j), 1)[0] - want).max() <= 1e-7
    finally:
        _lib.set_global_option("remove_block_rows", 0)
        g.close()
