"""GPU: the typed, strided query argument of mi_knn_search_grouped fed each layout of tests/_layouts.py, as
tests/test_gpu_input_layouts.py feeds the other searches on raw rows: every output (ids, scores, labels) must equal, byte for byte,
the answer for the contiguous float32 array, on "group_path" 1 and 2; that answer is pinned to the walk of tests/_grouped_truth.py
over the lattice ranking; float64 input that float32 cannot hold gives the answer of its float32 rounding.

Integer-lattice rows in a NORM_NONE gallery: every score is exact, so everything is asserted with ==.  Both paths ingest the queries
through mi_knn_search's staging (search_sync, launch_ingest of api_schedule.hip) and the fallback's host gather of re-run queries
(api_group.hip), which address base + i rs + j cs only: the broadcast layout (rs = 0) is included."""
import numpy as np
import pytest

import _grouped_truth as gt
import _lattice_truth as lt
import _layouts as L

pytestmark = pytest.mark.gpu

N, K = 600, 10
CASES = [(70, 37), (1, 130), (70, 130), (70, 1), (1, 1)]       # (nq, d) of tests/test_gpu_input_layouts.py


@pytest.fixture(scope="module")
def lib():
    return L.load_lib()


def _queries(nq, d):
    rng = np.random.default_rng(1000 * nq + d)
    mag = rng.integers(1, lt.HI + 1, size=(nq, d))              # no zero: beyond_float32 plants relative offsets
    return (mag * rng.choice([-1, 1], size=(nq, d))).astype(np.float32)


class Ctx:
    """One width: lattice rows, random groups of 1 .. 7 rows and one group of half the rows (so that collapsing changes every
    answer), and an exclude label per query"""

    def __init__(self, lib, d):
        rng = np.random.default_rng(d + 11)
        self.X = rng.integers(lt.LO, lt.HI + 1, size=(N, d)).astype(np.float32)
        self.labels = gt.random_labels(rng, N, spread=5)
        self.labels[rng.choice(N, 300, replace=False)] = 3
        self.g = lib.Gallery.from_host(self.X, norm_mode=lib.NORM_NONE)
        assert self.g.get_rows(0, N).tobytes() == self.X.tobytes(), "the gallery does not hold the rows it was given"
        self.g.set_groups(self.labels)

    def exclude(self, nq):
        return self.labels[np.random.default_rng(nq).integers(0, N, nq)]

    def call(self, x, path):
        self.g.set_option("group_path", path)
        try:
            idx, sc, _, lab = self.g.search_grouped(x, K, self.exclude(x.shape[0]), return_labels=True)
        finally:
            self.g.set_option("group_path", 0)
        return idx, sc, lab


@pytest.fixture(scope="module")
def ctxs(lib):
    made = {}

    def get(d):
        if d not in made:
            made[d] = Ctx(lib, d)
        return made[d]
    yield get
    for c in made.values():
        c.g.close()


@pytest.mark.parametrize("path", [1, 2])
def test_query_layouts_give_the_contiguous_answer(lib, ctxs, path):
    for nq, d in CASES:
        c = ctxs(d)
        q = _queries(nq, d)
        want = c.call(q, path)
        for lay in L.layouts(q, np.nan, bcast=True):
            ref = want if lay.name != "bcast32" else c.call(L.expected(lay, q), path)
            L.same(c.call(lay.view, path), ref, "mi_knn_search_grouped, path %d, %d x %d, %s" % (path, nq, d, lay.name))


@pytest.mark.parametrize("path", [1, 2])
def test_contiguous_query_answer_is_the_truth(lib, ctxs, path):
    for nq, d in CASES:
        c = ctxs(d)
        q = _queries(nq, d)
        ids, sc, lab = gt.grouped_truth(*gt.lattice_ranking(c.X, q), c.labels, K, c.exclude(nq))
        got = c.call(q, path)
        assert np.array_equal(got[0], ids) and got[1].tobytes() == sc.tobytes() and np.array_equal(got[2], lab)


@pytest.mark.parametrize("path", [1, 2])
def test_float64_queries_beyond_float32_are_rounded(lib, ctxs, path):
    for nq, d in CASES:
        c = ctxs(d)
        q = _queries(nq, d)
        q64 = L.beyond_float32(q, [0, nq - 1], [0, d - 1])
        want = c.call(q, path)
        L.same(c.call(q64, path), want, "mi_knn_search_grouped, path %d, %d x %d, float64 beyond float32" % (path, nq, d))
        for lay in L.layouts(q, np.nan):                       # the planted values through a strided float64 view
            if lay.name == "col64":
                lay.view[...] = q64
                L.same(c.call(lay.view, path), want, "mi_knn_search_grouped, path %d, %d x %d, float64 beyond float32, col64"
                       % (path, nq, d))
