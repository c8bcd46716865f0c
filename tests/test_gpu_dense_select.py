"""GPU: the selection kernels of csrc/dense.hip (dense_topk_kernel, dense_topk64_kernel, rank_all_kernel,
rank_positions_kernel) against an exact numpy sort, through the public entry points.

Every score here is known bit for bit.  The exact f32 scorer is a k-ordered fmaf chain that starts at +0
(csrc/exact_score.hip), and the f64 dense scorer is the same chain in f64.  So with an MI_NORM_NONE gallery G and the
unit query e_j, score[j, r] = G[r, j] + 0.0: the products with 0 add +-0 to the chain and change nothing, and the
starting +0 turns a stored -0 into +0.  Columns that hold NaN or +-inf go into d = 1 galleries queried with [1.0],
because 0 * inf would poison the other columns.

The reference is `np.argsort(-v, kind="stable")`: score descending, exact ties to the lower row, NaN last (NaN rows
by row ascending) -- the order the header and DESIGN give for all four kernels.  No tolerance anywhere."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OFF = 1000                       # row_offset of the galleries below (so that row_offset - 1 is not the padding id -1)
BIG_OFF = 3_000_000_000          # above 2**31: any 32-bit truncation of an output id shows


@pytest.fixture(scope="module")
def lib():
    from isehr_amd import _lib
    _lib.load()
    return _lib


# ---- value families: (rng, n) -> float32 [n] ------------------------------------------------------------------------

def fam_normal(rng, n):
    return rng.standard_normal(n).astype(np.float32)


def fam_negative(rng, n):
    return (-np.abs(rng.standard_normal(n)) - 1e-3).astype(np.float32)


def fam_quantised(rng, n):
    # ~16 levels: the tie group at the k-th value spans many rows and is cut part-way
    return (rng.integers(0, 16, n) * 0.375 - 2.5).astype(np.float32)


def fam_equal(rng, n):
    return np.full(n, 0.625, dtype=np.float32)


def fam_ulps(rng, n):
    # 1.5 + a permutation of i ulps: only the low radix digits differ
    return (np.uint32(0x3FC00000) + rng.permutation(n).astype(np.uint32)).view(np.float32)


def fam_subnormal(rng, n):
    # subnormals of both signs mixed with +0 and -0 (the scorer turns -0 into +0)
    mag = rng.integers(0, 1 << 23, n).astype(np.uint32)
    mag[rng.random(n) < 0.2] = 0
    sign = (rng.random(n) < 0.5).astype(np.uint32) << np.uint32(31)
    return (mag | sign).view(np.float32)


FINITE_FAMILIES = [fam_normal, fam_negative, fam_quantised, fam_equal, fam_ulps, fam_subnormal]


def fam_inf(rng, n):
    v = fam_quantised(rng, n)
    u = rng.random(n)
    v[u < 0.05] = np.inf
    v[(u >= 0.05) & (u < 0.1)] = -np.inf
    return v


def fam_nan(rng, n, n_real):
    """n_real non-NaN rows (normals with some +-inf) at random places, NaN everywhere else."""
    v = np.full(n, np.nan, dtype=np.float32)
    real = rng.choice(n, size=min(n, n_real), replace=False)
    r = fam_normal(rng, len(real))
    u = rng.random(len(real))
    r[u < 0.1] = np.inf
    r[(u >= 0.1) & (u < 0.2)] = -np.inf
    v[real] = r
    return v


# ---- helpers ---------------------------------------------------------------------------------------------------------

def scored(col):
    """What the scorer returns for a stored column queried by its unit vector: the value + 0.0 (-0 -> +0)."""
    return col + np.float32(0.0)


def ref_order(v):
    return np.argsort(-v, kind="stable")


def assert_same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want, dtype=got.dtype)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), "%s: NaN at different places (first %s)" % (what, np.flatnonzero(gn != wn)[:5])
    ut = np.uint32 if got.dtype == np.float32 else np.uint64
    bad = np.flatnonzero((got.view(ut) != want.view(ut)) & ~gn)
    assert len(bad) == 0, "%s: %d scores differ, first at %d: %r != %r" % (what, len(bad), bad[0], got[bad[0]],
                                                                           want[bad[0]])


def assert_ids(got, want, what):
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, "%s: %d ids differ, first at %d: got %d, want %d (got[:8] = %s)" % (
        what, len(bad), bad[0], got[bad[0]], want[bad[0]], got[:8].tolist())


def make_gallery(lib, cols, row_offset=OFF):
    """MI_NORM_NONE gallery whose column j is cols[j]; -> (gallery, unit queries [m, m], scored values [m, n])."""
    g = np.ascontiguousarray(np.stack(cols, axis=1).astype(np.float32))
    # MI_NORM_NONE stores the rows as given, non-finite values included (no check refuses them); the tests below rely on it
    G = lib.Gallery.from_host(g, norm_mode=lib.NORM_NONE, row_offset=row_offset)
    assert G.n == g.shape[0] and G.d == g.shape[1] and G.row_offset == row_offset
    return G, np.eye(g.shape[1], dtype=np.float32), np.stack([scored(c) for c in cols])


def check_dense(G, q, vals, k, path, row_offset):
    if path == "dense":
        idx, sc, _ = G.dense_search(q, k)
        sc64 = None
    else:
        idx, sc, sc64, _ = G.dense64_search(q, k)
    assert idx.shape == (len(q), k)
    for j in range(len(q)):
        o = ref_order(vals[j])[:k]
        what = "%s query %d k=%d n=%d" % (path, j, k, len(vals[j]))
        assert_ids(idx[j], o + row_offset, what)
        assert_same_bits(sc[j], vals[j][o], what + " f32 scores")
        if sc64 is not None:
            assert_same_bits(sc64[j], vals[j][o].astype(np.float64), what + " f64 scores")


# ---- dense top-k: dense_topk_kernel (mi_knn_dense_search) and dense_topk64_kernel (mi_knn_dense64_search) --------------

DENSE_K = [1, 2, 3, 63, 64, 65, 255, 256, 257, 1000, 2047, 2048, 2049, 4095, 4096]
DENSE_CASES = [(k, n) for k in DENSE_K for n in sorted({k, k + 1, 5000, 70000}) if n >= k]


@pytest.mark.parametrize("path", ["dense", "dense64"])
@pytest.mark.parametrize("k,n", DENSE_CASES)
def test_dense_topk_exact(lib, path, k, n):
    rng = np.random.default_rng(1000 * k + n)
    # six finite families side by side: one query (one workgroup) per family
    G, q, vals = make_gallery(lib, [f(rng, n) for f in FINITE_FAMILIES])
    try:
        check_dense(G, q, vals, k, path, OFF)
    finally:
        G.close()
    # +-inf among quantised values
    G, q, vals = make_gallery(lib, [fam_inf(rng, n)])
    try:
        check_dense(G, q, vals, k, path, OFF)
    finally:
        G.close()
    # fewer than k non-NaN rows: the top-k ends in NaN rows, by row ascending
    G, q, vals = make_gallery(lib, [fam_nan(rng, n, k // 2)])
    try:
        check_dense(G, np.ones((2, 1), np.float32), np.repeat(vals, 2, axis=0), k, path, OFF)
    finally:
        G.close()


@pytest.mark.parametrize("path", ["dense", "dense64"])
def test_dense_topk_all_nan_rows(lib, path):
    """Every score NaN: the k outputs are rows 0..k-1, scores NaN -- for a k that is a power of two and for ones that
    are not (the LDS sort array is padded from k up to the next power of two)."""
    G, _, _ = make_gallery(lib, [np.full(300, np.nan, np.float32)])
    try:
        for k in (1, 5, 64, 100, 300):
            if path == "dense":
                idx, sc, _ = G.dense_search(np.ones((3, 1), np.float32), k)
            else:
                idx, sc, _, _ = G.dense64_search(np.ones((3, 1), np.float32), k)
            for j in range(3):
                assert_ids(idx[j], np.arange(k) + OFF, "%s k=%d" % (path, k))
            assert np.isnan(sc).all()
    finally:
        G.close()


@pytest.mark.parametrize("path", ["dense", "dense64"])
def test_dense_topk_rejects_bad_k(lib, path):
    rng = np.random.default_rng(5)
    for n, k in ((100, 101), (5000, 4097), (5000, 0)):
        G, q, _ = make_gallery(lib, [fam_normal(rng, n)])
        try:
            with pytest.raises(RuntimeError):
                if path == "dense":
                    G.dense_search(q, k)
                else:
                    G.dense64_search(q, k)
        finally:
            G.close()


# ---- full ranking: rank_all_kernel (mi_rank_all, mi_rank_prefix) and rank_positions_kernel (mi_rank_positions) ---------

RANK_N = [1, 2, 15, 16, 17, 63, 64, 65, 1023, 1025, 4097, 70001]


def listed_ids(rng, n, m, v, row_offset):
    """m global ids for mi_rank_positions: rows of the shard (duplicates, NaN rows, members of the largest tie group,
    the first and last row), the padding id -1 and the ids just outside the shard."""
    special = [row_offset - 1, -1, row_offset + n, row_offset, row_offset + n - 1]
    nan_rows = np.flatnonzero(np.isnan(v))
    _, inv, cnt = np.unique(np.where(np.isnan(v), np.inf, v), return_inverse=True, return_counts=True)
    tie_rows = np.flatnonzero(inv == np.argmax(cnt))
    pool = [rng.integers(0, n, m)]
    if len(nan_rows):
        pool.append(rng.choice(nan_rows, m))
    pool.append(rng.choice(tie_rows, m))
    picks = np.concatenate(pool)[rng.permutation(m * len(pool))][:m] + row_offset
    ids = np.concatenate([special, picks])[:m] if m > 1 else picks[:1]
    if m > 2:
        ids[-1] = ids[-2]                                   # a duplicate
    return rng.permutation(ids).astype(np.int64)


def check_rank(G, q, vals, row_offset, rng):
    n = vals.shape[1]
    orders = [ref_order(v) for v in vals]
    full, sc, _ = G.rank_all(q, return_scores=True)
    assert full.shape == (len(q), n)
    for j, o in enumerate(orders):
        assert_ids(full[j], o + row_offset, "rank_all query %d n=%d" % (j, n))
        assert_same_bits(sc[j], vals[j][o], "rank_all query %d n=%d scores" % (j, n))
    for keep in sorted({1, n // 2, n} - {0}):
        pre, psc, _ = G.rank_prefix(q, keep, return_scores=True)
        assert pre.shape == (len(q), keep)
        for j, o in enumerate(orders):
            assert_ids(pre[j], o[:keep] + row_offset, "rank_prefix query %d n=%d keep=%d" % (j, n, keep))
            assert_same_bits(psc[j], vals[j][o[:keep]], "rank_prefix query %d n=%d keep=%d scores" % (j, n, keep))
    for m in (1, 7, 2048):
        ids = np.stack([listed_ids(rng, n, m, v, row_offset) for v in vals])
        pos = G.rank_positions(q, ids)
        for j, o in enumerate(orders):
            where = np.empty(n, np.int64)
            where[o] = np.arange(n)
            local = ids[j] - row_offset
            inside = (local >= 0) & (local < n)
            want = np.full(m, -1, np.int64)
            want[inside] = where[local[inside]]
            assert_ids(pos[j], want, "rank_positions query %d n=%d m=%d" % (j, n, m))
    with pytest.raises(RuntimeError):
        G.rank_positions(q, np.full((len(q), 2049), row_offset, np.int64))


@pytest.mark.parametrize("n", RANK_N)
def test_rank_all_prefix_positions_exact(lib, n):
    """Full stable argsort, including ties that span the 16 wave segments of rank_all_kernel (all-equal and quantised
    columns) and n below 16 (empty segments)."""
    rng = np.random.default_rng(77 + n)
    G, q, vals = make_gallery(lib, [f(rng, n) for f in FINITE_FAMILIES])
    try:
        check_rank(G, q, vals, OFF, rng)
    finally:
        G.close()
    # NaN rows (a third), +-inf among the rest
    G, q, vals = make_gallery(lib, [fam_nan(rng, n, n - n // 3)])
    try:
        check_rank(G, q, vals, OFF, rng)
    finally:
        G.close()


# ---- row_offset above 2**31 through all four entry points ---------------------------------------------------------------

def test_row_offset_above_2_pow_31(lib):
    rng = np.random.default_rng(31)
    n = 5000
    for cols in ([f(rng, n) for f in FINITE_FAMILIES], [fam_nan(rng, n, 200)]):
        G, q, vals = make_gallery(lib, cols, row_offset=BIG_OFF)
        try:
            for k in (1, 257, 4096):
                check_dense(G, q, vals, k, "dense", BIG_OFF)
                check_dense(G, q, vals, k, "dense64", BIG_OFF)
            check_rank(G, q, vals, BIG_OFF, rng)
        finally:
            G.close()


# ---- product level: a zero query under MI_NORM_L2 normalises to a NaN row, so every one of its scores is NaN ----------

@pytest.mark.parametrize("k", [1, 20, 100, 129])
def test_zero_query_dense_paths(lib, k):
    from isehr_amd.synth import synth_rows
    g = synth_rows(7, 0, 3000, 96)
    q = synth_rows(8, 0, 3, 96)
    q[1] = 0.0
    G = lib.Gallery.from_host(g, norm_mode=lib.NORM_L2, row_offset=OFF)
    try:
        with np.errstate(all="ignore"):
            idx, sc, _ = G.dense_search(q, k)
            idx64, sc64, s64, _ = G.dense64_search(q, k)
    finally:
        G.close()
    for got, s in ((idx, sc), (idx64, sc64), (idx64, s64)):
        assert_ids(got[1], np.arange(k) + OFF, "zero query k=%d" % k)
        assert np.isnan(s[1]).all()
        for j in (0, 2):                                    # the other queries of the batch are untouched
            assert len(set(got[j].tolist())) == k and got[j].min() >= OFF and got[j].max() < OFF + 3000
            assert not np.isnan(s[j]).any()
