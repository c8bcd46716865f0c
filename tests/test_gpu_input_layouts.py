"""GPU: every typed, strided entry point that works on raw rows (galleries, the exact searches, refine, graph, forest), fed each
layout of tests/_layouts.py.  Every output must equal, byte for byte, the answer for the contiguous float32 array; that answer is
itself pinned to the feature's own truth (tests/_lattice_truth.py, _refine_truth.py, _graph_truth.py, _forest_truth.py).

The data is the integer lattice of _lattice_truth.py in NORM_NONE and squared-L2 galleries: every score and every distance is
exact in every number format and summation order, so all truths are asserted with ==.  This is the family whose header sentence
is "f64 rounded to f32": float64 input that float32 cannot hold must give the answer of its float32 rounding.

At these widths (1, 37, 130) the gallery rows go through the generic instantiations of ingest_rows_kernel and the transposing
scratch path only: the vectorised branch (d a multiple of 4, 16-byte rows) and ingest_cols_kernel (d = 2048, rs = 1) are not
reached here; tests/test_gpu_ingest_bits.py sweeps those."""
import ctypes as C

import numpy as np
import pytest

import _forest_truth as FT
import _graph_truth as GT
import _lattice_truth as lt
import _layouts as L
import _refine_truth as RT
from _diffusion_checks import check_online, clustered

pytestmark = pytest.mark.gpu

N, K, EF, R_GRAPH, KC = 600, 10, 16, 8, 32
TREES, LEVELS = 3, 4
DIF_T, DIF_KD, DIF_KQ, DIF_GAMMA = 50, 10, 3, 3
# (nq, d): one query and 70 (across the 16-query blocks and the 64-lane wave); widths 1, 37 and 130
CASES = [(70, 37), (1, 130), (70, 130), (70, 1), (1, 1)]
DATA_DS = [37, 130, 1]


@pytest.fixture(scope="module")
def lib():
    return L.load_lib()


def _lattice(seed, n, d):
    return np.random.default_rng(seed).integers(lt.LO, lt.HI + 1, size=(n, d)).astype(np.float32)


def _queries(nq, d):
    rng = np.random.default_rng(1000 * nq + d)
    mag = rng.integers(1, lt.HI + 1, size=(nq, d))                          # no zero: beyond_float32 plants relative offsets
    return (mag * rng.choice([-1, 1], size=(nq, d))).astype(np.float32)


class Ctx:
    """The handles of one width d, built once: a NORM_NONE gallery and a squared-L2 gallery of the same lattice rows, a graph and a
    forest over the L2 gallery."""

    def __init__(self, lib, d):
        self.lib, self.d = lib, d
        self.X = _lattice(d, N, d)
        self.g = lib.Gallery.from_host(self.X, norm_mode=lib.NORM_NONE)
        self.gl2 = lib.Gallery.l2_from_host(self.X)
        for g in (self.g, self.gl2):
            assert GT.gallery_rows(g).tobytes() == self.X.tobytes(), "the gallery does not hold the rows it was given"
        self.graph = lib.GraphIndex.build(self.gl2, R=R_GRAPH, n_entry=4)
        rng = np.random.default_rng(d + 5)
        self.dirs = rng.standard_normal((TREES * LEVELS, d))
        self.splits = rng.standard_normal((TREES, (1 << LEVELS) - 1)) * 2.0
        self.leaves = np.stack([rng.permutation(N) for _ in range(TREES)]).astype(np.int32)
        self.forest = lib.ForestIndex.from_trees(self.gl2, self.dirs, self.splits, self.leaves)
        self.mask = np.random.default_rng(d + 6).random(N) < 0.4

    def close(self):
        for h in (self.forest, self.graph, self.gl2, self.g):
            h.close()


@pytest.fixture(scope="module")
def ctxs(lib):
    made = {}

    def get(d):
        if d not in made:
            made[d] = Ctx(lib, d)
        return made[d]
    yield get
    for c in made.values():
        c.close()


def _src(lib, x):
    """(pointer, dtype code, row stride, col stride, memspace) of a numpy view (never copied) or a torch device tensor."""
    if isinstance(x, np.ndarray):
        a, code, rs, cs = lib._strided(x)
        assert a is x or a.ctypes.data == x.ctypes.data, "the binding copied a layout it should pass through"
        return x.ctypes.data, code, rs, cs, lib.MI_HOST
    import torch
    code = lib.MI_F32 if x.dtype == torch.float32 else lib.MI_F64
    return x.data_ptr(), code, x.stride(0), x.stride(1), lib.MI_DEVICE


def _cand(nq):
    c = np.random.default_rng(nq).integers(0, N, size=(nq, KC)).astype(np.int64)
    c[:, 3] = -1                                                            # padding
    c[:, 5] = c[:, 4]                                                       # a repeat
    return c


def _tau(c, q):
    """an integer threshold a few dozen rows per query pass"""
    return float(np.sort(lt.int_scores(c.X, np.ascontiguousarray(q, np.float32)).ravel())[-min(40 * len(q), N * len(q) // 4)])


class DiffusionCtx:
    """A MI_NORM_NONE gallery of clustered unit rows with the offline diffusion result it computed itself (what
    tests/test_gpu_diffusion_exact.py pins), for mi_diffusion_online.  Width 1 is left out: unit rows of one column are +-1, every
    similarity ties and the kNN graph says nothing."""

    def __init__(self, lib, d):
        self.f = clustered(300 + d, N, d)
        self.G = lib.Gallery.from_host(self.f, norm_mode=lib.NORM_NONE)
        self.ids, self.vals = self.G.diffusion_offline(DIF_T, DIF_KD)

    def queries(self, nq):
        """perturbed gallery rows, used as given"""
        from isehr_amd.synth import synth_rows
        d = self.f.shape[1]
        base = self.f[(np.arange(nq) * 37) % N].astype(np.float64)
        return (base + 0.25 * synth_rows(nq + d, 0, nq, d).astype(np.float64) / np.sqrt(d)).astype(np.float32)

    def close(self):
        self.G.close()


@pytest.fixture(scope="module")
def difs(lib):
    made = {}

    def get(d):
        if d not in made:
            made[d] = DiffusionCtx(lib, d)
        return made[d]
    yield get
    for c in made.values():
        c.close()


# ---- the table: name -> (call, truth).  call(c, x) -> tuple of arrays; truth(c, q, out) asserts the contiguous answer ----------
def _topk_truth(c, q, out, k=K, mask=None):
    S = lt.int_scores(c.X, q)
    ids, sc = lt.filtered_truth(S, np.ones(N, bool) if mask is None else mask, k)
    assert np.array_equal(out[0], ids) and out[1].tobytes() == sc.tobytes()
    return S, ids


def _sqdist(c, q):
    Xi, Qi = c.X.astype(np.int64), q.astype(np.int64)
    return ((Qi[:, None, :] - Xi[None, :, :]) ** 2).sum(-1)


def _l2_truth(c, q, out):
    D = _sqdist(c, q)
    ids = lt.filtered_truth(-D, np.ones(N, bool), K)[0]
    assert np.array_equal(out[0], ids)
    assert out[1].tobytes() == np.take_along_axis(D, ids, 1).astype(np.float32).tobytes()
    assert out[2].tobytes() == np.take_along_axis(D, ids, 1).astype(np.float64).tobytes()


def _dense64_truth(c, q, out):
    S, ids = _topk_truth(c, q, out)
    assert out[2].tobytes() == np.take_along_axis(S, ids, 1).astype(np.float64).tobytes()


def _range_truth(c, q, out):
    lims, ids, sc = lt.range_truth(lt.int_scores(c.X, q), _tau(c, q))
    assert np.array_equal(out[0], lims) and np.array_equal(out[1], ids) and out[2].tobytes() == sc.tobytes()
    assert lims[-1] > 0


def _positions_truth(c, q, out):
    S = lt.int_scores(c.X, q)
    rank_ids = lt.filtered_truth(S, np.ones(N, bool), N)[0]
    pos = np.argsort(rank_ids, axis=1)                                      # pos[q, row] = position of row
    want = np.where(_cand(len(q)) >= 0, np.take_along_axis(pos, np.maximum(_cand(len(q)), 0), 1), -1)
    assert np.array_equal(out[0], want)


def _refine_truth(c, q, out):
    for o, l2 in ((out[:3], False), (out[3:], True)):
        ids, val = RT.refine_truth(c.X, q, _cand(len(q)), K, l2)
        assert np.array_equal(o[0], ids) and o[2].tobytes() == val.tobytes() and o[1].tobytes() == val.astype(np.float32).tobytes()


def _graph_truth(c, q, out):
    ids, val, vis = GT.search_truth(_sqdist(c, q).astype(np.float64), c.graph.neighbors, c.graph.entries, K, EF, True)
    assert np.array_equal(out[0], ids) and out[2].tobytes() == val.tobytes() and np.array_equal(out[3], vis)
    assert out[1].tobytes() == val.astype(np.float32).tobytes()


def _forest_cand_truth(c, q, out):
    want = FT.candidates_truth(FT.project(np.asarray(q, np.float32), c.dirs), c.splits, c.leaves, N, TREES, LEVELS, 0)
    assert np.array_equal(out[0], want)
    return want


def _forest_truth(c, q, out):
    cand = c.forest.candidates(q)
    _forest_cand_truth(c, q, (cand,))
    ids, val = RT.refine_truth(c.X, q, cand, K, True)
    assert np.array_equal(out[0], ids) and out[1].tobytes() == val.tobytes()


def _graph_call(c, x):
    p, code, rs, cs, _ = _src(c.lib, x)
    nq = x.shape[0]
    ids, v32, v64 = np.empty((nq, K), np.int64), np.empty((nq, K), np.float32), np.empty((nq, K), np.float64)
    vis = np.empty(nq, np.int32)
    c.lib.check(c.lib.load().mi_graph_search(c.graph._h, C.c_void_p(p), nq, code, rs, cs, K, EF, ids.ctypes.data, v32.ctypes.data,
                                             v64.ctypes.data, vis.ctypes.data, None))
    return ids, v32, v64, vis


QUERY_ROWS = {
    "mi_knn_search": (lambda c, x: c.g.search(x, K)[:2], _topk_truth),
    "mi_knn_search_filtered": (lambda c, x: c.g.search_filtered(x, K, allow=c.mask)[:2],
                               lambda c, q, out: _topk_truth(c, q, out, mask=c.mask)),
    "mi_range_search": (lambda c, x: c.g.range_search(x, _tau(c, x))[:3], _range_truth),
    "mi_knn_dense_search": (lambda c, x: c.g.dense_search(x, K)[:2], _topk_truth),
    "mi_knn_dense64_search": (lambda c, x: c.g.dense64_search(x, K)[:3], _dense64_truth),
    "mi_rank_all": (lambda c, x: c.g.rank_all(x, return_scores=True)[:2], lambda c, q, out: _topk_truth(c, q, out, k=N)),
    "mi_rank_prefix": (lambda c, x: c.g.rank_prefix(x, K, return_scores=True)[:2], _topk_truth),
    "mi_rank_positions": (lambda c, x: (c.g.rank_positions(x, _cand(x.shape[0])),), _positions_truth),
    "mi_knn_search_l2": (lambda c, x: c.gl2.search_l2(x, K)[:3], _l2_truth),
    "mi_knn_dense64_search_l2": (lambda c, x: c.gl2.dense64_search_l2(x, K)[:3], _l2_truth),
    "mi_refine": (lambda c, x: c.g.refine(x, _cand(x.shape[0]), K)[:3] + c.gl2.refine(x, _cand(x.shape[0]), K)[:3], _refine_truth),
    "mi_graph_search": (_graph_call, _graph_truth),
    "mi_forest_candidates": (lambda c, x: (c.forest.candidates(x),), _forest_cand_truth),
    "mi_forest_search": (lambda c, x: c.forest.search(x, K, return_values64=True)[:2], _forest_truth),
}


def _stored(lib, g):
    try:
        return (GT.gallery_rows(g), np.array([g.n, g.d], np.int64))
    finally:
        g.close()


def _create(lib, x, l2):
    """mi_gallery_create_l2, or mi_gallery_create under MI_NORM_NONE (outputs 0, 1) and under MI_NORM_L2 (outputs 2, 3: the
    normalising ingest, whose values test_gpu_ingest_bits.py pins; here every layout and float64 holding float32 must give its bits)"""
    p, code, rs, cs, mem = _src(lib, x)
    h = C.c_void_p()
    if l2:
        lib.check(lib.load().mi_gallery_create_l2(C.c_void_p(p), x.shape[0], x.shape[1], code, rs, cs, mem, 0, 0, 0, C.byref(h)))
        return _stored(lib, lib.Gallery(h.value))
    out = ()
    for mode in (lib.NORM_NONE, lib.NORM_L2):
        lib.check(lib.load().mi_gallery_create(C.c_void_p(p), x.shape[0], x.shape[1], code, rs, cs, mem, mode, 0, 0, C.byref(h)))
        out += _stored(lib, lib.Gallery(h.value))
    return out


def _append(lib, x):
    """two appends (the second starts at a row that is no multiple of 4 or 256) into an empty NORM_NONE gallery and into an empty
    squared-L2 gallery"""
    p, code, rs, cs, mem = _src(lib, x)
    esz = 4 if code == lib.MI_F32 else 8
    n, d = x.shape
    cut = min(n - 1, 257)                                                   # (a single row: one append)
    out = ()
    for g in (lib.Gallery.empty(n, d, norm_mode=lib.NORM_NONE), lib.Gallery.l2_from_host(None, capacity=n, d=d)):
        try:
            for r0, m in ((0, cut), (cut, n - cut))[0 if cut else 1:]:
                lib.check(lib.load().mi_gallery_append(g._h, C.c_void_p(p + r0 * rs * esz), m, code, rs, cs, mem))
                g.n += m
        except BaseException:
            g.close()
            raise
        out += _stored(lib, g)
    return out


def _rows_truth(a, out, stored_as_given=None):
    """the galleries that store their rows as given (all but the MI_NORM_L2 one of mi_gallery_create) hold `a` bit for bit"""
    for i, (rows, shape) in enumerate(zip(out[0::2], out[1::2])):
        assert tuple(shape) == a.shape
        if stored_as_given is None or i < stored_as_given:
            assert rows.tobytes() == a.tobytes()
        else:
            norms = np.sqrt((rows.astype(np.float64) ** 2).sum(1))
            assert (np.abs(norms[(a != 0).any(1)] - 1.0) <= 1e-6).all()      # (a sanity check only; the values: test_gpu_ingest_bits.py)


DATA_ROWS = {
    "mi_gallery_create": (lambda lib, x: _create(lib, x, False), lambda a, out: _rows_truth(a, out, 1)),
    "mi_gallery_create_l2": (lambda lib, x: _create(lib, x, True), _rows_truth),
    "mi_gallery_append": (_append, _rows_truth),
}

ROWS = {**QUERY_ROWS, **DATA_ROWS, "mi_diffusion_online": None}          # (its tests stand at the end of the file)


_same = L.same


@pytest.mark.parametrize("name", sorted(QUERY_ROWS))
def test_query_layouts_give_the_contiguous_answer(lib, ctxs, name):
    """host memory (these entry points take no memspace); bcast32 (rs = 0) included: every query ingest behind these entry points
    addresses base + i rs + j cs only (ingest.hip ingest_query_kernel / ingest_rows_kernel, l2_metric.hip l2_augment_kernel,
    forest_project.hip, api_filter.hip's host gather)"""
    call = QUERY_ROWS[name][0]
    for nq, d in CASES:
        c = ctxs(d)
        q = _queries(nq, d)
        want = call(c, q)
        for lay in L.layouts(q, np.nan, bcast=True):
            ref = want if lay.name != "bcast32" else call(c, L.expected(lay, q))
            _same(call(c, lay.view), ref, "%s, %d x %d, %s" % (name, nq, d, lay.name))


@pytest.mark.parametrize("name", sorted(QUERY_ROWS))
def test_contiguous_query_answer_is_the_truth(lib, ctxs, name):
    call, truth = QUERY_ROWS[name]
    for nq, d in CASES:
        c = ctxs(d)
        q = _queries(nq, d)
        truth(c, q, call(c, q))


@pytest.mark.parametrize("name", sorted(QUERY_ROWS))
def test_float64_queries_beyond_float32_are_rounded(lib, ctxs, name):
    """"f64 rounded to f32" (include/mi355_retrieval.h): the answer for a64 is the answer for a64.astype(float32), bit for bit"""
    call = QUERY_ROWS[name][0]
    for nq, d in CASES:
        c = ctxs(d)
        q = _queries(nq, d)
        q64 = L.beyond_float32(q, [0, nq - 1], [0, d - 1])
        _same(call(c, q64), call(c, q), "%s, %d x %d, float64 beyond float32" % (name, nq, d))
        for lay in L.layouts(q, np.nan):                                   # the planted values through a strided float64 view
            if lay.name == "col64":
                lay.view[...] = q64
                _same(call(c, lay.view), call(c, q), "%s, %d x %d, float64 beyond float32, col64" % (name, nq, d))


@pytest.mark.parametrize("name", sorted(DATA_ROWS))
def test_data_layouts_give_the_contiguous_answer(lib, name):
    """each layout once from host memory and once from device memory"""
    import torch
    call, truth = DATA_ROWS[name]
    for d in DATA_DS:
        a = _lattice(d + 50, N, d)
        want = call(lib, a)
        truth(a, want)
        for lay in L.layouts(a, np.nan):
            _same(call(lib, lay.view), want, "%s, %d x %d, %s, host" % (name, N, d, lay.name))
            t = L.on_device(lay)
            torch.cuda.synchronize()
            _same(call(lib, t), want, "%s, %d x %d, %s, device" % (name, N, d, lay.name))
    one = _lattice(3, 1, 37)                                                # a single row: numpy reports the parent's strides
    one[one == 0] = 1
    want = call(lib, one)
    truth(one, want)
    for lay in L.layouts(one, np.nan):
        _same(call(lib, lay.view), want, "%s, 1 x 37, %s, host" % (name, lay.name))
        t = L.on_device(lay)
        torch.cuda.synchronize()
        _same(call(lib, t), want, "%s, 1 x 37, %s, device" % (name, lay.name))


@pytest.mark.parametrize("name", sorted(DATA_ROWS))
def test_float64_data_beyond_float32_is_rounded(lib, name):
    call = DATA_ROWS[name][0]
    a = _lattice(77, N, 37)
    a[a == 0] = 1
    a64 = L.beyond_float32(a, [0, 255, 256, N - 1], [0, 36])
    # (under MI_NORM_L2 such values are scaled in float64 before the one rounding: outputs 2, 3 of mi_gallery_create are left out)
    keep = 2 if name == "mi_gallery_create" else None
    _same(call(lib, a64)[:keep], call(lib, a)[:keep], "%s, float64 beyond float32" % name)


def test_negative_strides_are_refused(lib, ctxs):
    c = ctxs(37)
    q = _queries(3, 37)
    ids = np.empty((3, K), np.int64)
    rc = lib.load().mi_knn_search(c.g._h, C.c_void_p(q.ctypes.data), 3, lib.MI_F32, -37, 1, K, ids.ctypes.data, None, None)
    assert rc == lib.MI_ERR_INVALID
    rc = lib.load().mi_graph_search(c.graph._h, C.c_void_p(q.ctypes.data), 3, lib.MI_F32, 37, -1, K, EF, ids.ctypes.data, None, None,
                                    None, None)
    assert rc == lib.MI_ERR_INVALID


# ---- mi_diffusion_online: a handle of its own, the truth of tests/_diffusion_checks.py with its bound -------------------------
@pytest.mark.parametrize("nq,d", [(70, 37), (1, 130), (70, 130)])
def test_diffusion_online_layouts_truth_and_float64(lib, difs, nq, d):
    """every layout (bcast32 too: the query ingest is mi_knn_search's, search_sync of api_schedule.hip) gives the contiguous float32
    ranks and scores byte for byte; those pass check_online; float64 queries beyond float32 are rounded to float32 by the ingest
    (scale 1 under MI_NORM_NONE), so they give the answer of their rounding bit for bit"""
    c = difs(d)
    q = c.queries(nq)

    def call(x):
        return c.G.diffusion_online(x, DIF_KQ, DIF_GAMMA, DIF_T)
    want = call(q)
    check_online(c.G, c.f, c.ids, c.vals, q, DIF_KQ, DIF_GAMMA, DIF_T, want[0], want[1], label="layout sweep")
    for lay in L.layouts(q, np.nan, bcast=True):
        ref = want if lay.name != "bcast32" else call(L.expected(lay, q))
        _same(call(lay.view), ref, "mi_diffusion_online, %d x %d, %s" % (nq, d, lay.name))
    q64 = L.beyond_float32(q, [0, nq - 1], [0, d - 1])
    _same(call(q64), want, "mi_diffusion_online, %d x %d, float64 beyond float32" % (nq, d))
    for lay in L.layouts(q, np.nan):
        if lay.name in ("t64", "col64"):
            lay.view[...] = q64
            _same(call(lay.view), want, "mi_diffusion_online, %d x %d, float64 beyond float32, %s" % (nq, d, lay.name))
