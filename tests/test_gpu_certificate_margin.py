"""GPU: every consumer of the certificate's margin on data whose rounding errors attain the bound.

tests/_margin_truth.py plants, per query, K victims whose 16-bit score underestimates the exact one by |q^||g^ - g| and K
imposters whose 16-bit score overestimates it by as much: the 16-bit top-K is the imposters, the exact top-K is the victims, and
the lowest victim lies 0.95 ... 0.99 of the shipped margin below the K-th 16-bit score.  tests/test_margin_truth_cpu.py shows
that a filter applying 0.85 of the margin loses victims on exactly this data.  Every score is exact in every format and order, so
ids are compared with ==, scores as bits, and the gallery must hold the rows it was given bit for bit.  The statistics show that
the 16-bit path gave the answer: no overflowed batch, no speculative retry, and exactly the 2 K candidates per query the model
counts (the f32 scorer would keep K).  The two consumers this file leaves out have files of their own: the sharded protocol's
worst-shard margin (tests/test_gpu_certificate_margin_sharded.py) and search_l2, whose hidden columns make the 16-bit score depend
on the summation order, so that its model is banded (tests/test_gpu_certificate_margin_l2.py); DESIGN 3, "What pins the margin"."""
import numpy as np
import pytest

import _margin_truth as mt

pytestmark = pytest.mark.gpu

IDS = ["d%d-%s-n%d" % c[:3] for c in mt.CASES]
NQS = (1, 70, 128, 129, 300)          # the streaming kernel, the batch-size boundary between the two kernels, the tile kernel


@pytest.fixture(scope="module", params=mt.CASES, ids=IDS)
def case(request):
    from isehr_amd import _lib
    prob = mt.problem(*request.param)
    f16 = 1 if prob.image == "f16" else 0
    _lib.set_global_option("image_dtype", f16)
    try:
        g = _lib.Gallery.from_host(prob.X, norm_mode=_lib.NORM_NONE)
    finally:
        _lib.set_global_option("image_dtype", 1)
    try:
        assert int(g.get_option("image_dtype")) == f16, "the gallery took another image type"
        _stored(g, prob)
        bounds = np.array(g.norm_bounds(), np.float32)
        # the maxima the margin is made of: each within its 1e-6 inflation of the model's (summation order only)
        assert np.allclose(bounds, np.array(prob.norm_bounds(), np.float32), rtol=4e-7, atol=0)
        yield g, prob
    finally:
        g.close()


def _stored(g, prob):
    R = g.get_rows(0, g.n)
    assert g.n == prob.n and np.array_equal(R.view(np.uint32), prob.X.view(np.uint32)), "the gallery does not hold the rows it was given"


def _same_topk(ids, sc, want, what):
    wi, ws = want
    assert ids.dtype == np.int64 and ids.shape == wi.shape
    if not np.array_equal(ids, wi):
        q, j = (int(v[0]) for v in np.nonzero(ids != wi))
        lost = sorted(set(wi[q].tolist()) - set(ids[q].tolist()))
        raise AssertionError("%s: query %d, position %d: row %d, the truth has row %d; %d true rows are missing (first: %s)"
                             % (what, q, j, ids[q, j], wi[q, j], len(lost), lost[:5]))
    if sc.dtype == np.float64:
        assert np.array_equal(sc.view(np.uint64), ws.view(np.uint64)), "%s: float64 score bits differ" % what
    else:
        assert sc.dtype == np.float32 and np.array_equal(sc.view(np.uint32), ws.astype(np.float32).view(np.uint32)), \
            "%s: score bits differ" % what


class _Options:
    """sets handle options and puts back what they were"""

    def __init__(self, g, **opts):
        self.g, self.opts = g, opts

    def __enter__(self):
        self.old = {k: self.g.get_option(k) for k in self.opts}
        for k, v in self.opts.items():
            self.g.set_option(k, v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            self.g.set_option(k, v)


def _stats(g, what, nq=None, prob=None):
    """the 16-bit path gave the answer: no overflowed batch, no retry; with nq: exactly the candidates the model counts"""
    st = g.status(reset=True)
    print("\n%s: inkernel_repairs %d, survivors %d, candidates %d over %d queries"
          % (what, st["inkernel_repairs"], st["survivors"], st["candidates"], st["queries"]))
    assert st["overflow_batches"] == 0 and st["spec_retries"] == 0, (what, st)
    if nq is not None:
        assert st["candidates"] == int(prob.candidates()[prob.of_query(nq)].sum()), (what, st)
    return st


SETTINGS = [("defaults", {}), ("ladder off", {"ladder": 0}), ("rigorous chunk schedule", {"speculative": 0}),
            ("boot_ksplit off", {"boot_ksplit": 0}), ("boot_ksplit on", {"boot_ksplit": 1})]


@pytest.mark.parametrize("name, opts", SETTINGS, ids=[s[0].replace(" ", "_") for s in SETTINGS])
def test_search(case, name, opts):
    g, prob = case
    g.status(reset=True)
    for nq in NQS:
        Q, want = prob.queries(0, nq), prob.truth(nq=nq)
        what = "%s, %d queries" % (name, nq)
        with _Options(g, **opts):
            ids, sc, _ = g.search(Q, prob.k)
        _same_topk(ids, sc, want, what)
        _stats(g, what, nq, prob)
    assert (prob.candidates() == 2 * prob.k).all()


def test_force_exact_gives_the_same_bits(case):
    g, prob = case
    for nq in (1, 129):
        Q, want = prob.queries(0, nq), prob.truth(nq=nq)
        ids, sc, _ = g.search(Q, prob.k)
        with _Options(g, force_exact=1):
            ids_x, sc_x, _ = g.search(Q, prob.k)
        _same_topk(ids, sc, want, "16-bit path, %d queries" % nq)
        _same_topk(ids_x, sc_x, want, "force_exact, %d queries" % nq)
        assert np.array_equal(ids, ids_x) and np.array_equal(sc.view(np.uint32), sc_x.view(np.uint32))
    _stored(g, prob)


@pytest.mark.parametrize("nq", [1, 70])
def test_search_device(case, nq):
    """the asynchronous entry point (a small batch is repaired inside the maintain launch): the same answers, float64 bits"""
    import torch
    g, prob = case
    want = prob.truth(nq=nq)
    g.status(reset=True)
    q = torch.from_numpy(prob.queries(0, nq)).cuda()
    ix = torch.full((nq, prob.k), -7, dtype=torch.int64, device="cuda")
    s32 = torch.zeros((nq, prob.k), dtype=torch.float32, device="cuda")
    s64 = torch.zeros((nq, prob.k), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    g.search_device(q.data_ptr(), nq, prob.k, ix.data_ptr(), s32.data_ptr(), s64.data_ptr())
    g.join()
    torch.cuda.synchronize()
    assert g.flags() == 0
    _same_topk(ix.cpu().numpy(), s64.cpu().numpy(), want, "search_device, %d queries" % nq)
    _same_topk(ix.cpu().numpy(), s32.cpu().numpy(), want, "search_device, %d queries, float32" % nq)
    _stats(g, "search_device, %d queries" % nq, nq, prob)


@pytest.mark.parametrize("path", [0, 1, 2])
def test_search_filtered(case, path):
    """path 1 scores a sub-gallery of the allowed rows under the parent's norm maxima, path 2 over-fetches from the whole
    gallery, 0 chooses: each runs the 16-bit scoring launch"""
    g, prob = case
    g.status(reset=True)
    for name, allow in prob.allow_sets().items():
        for nq in (prob.patterns, 130):
            want = prob.truth(allow=allow, nq=nq)
            what = "filter_path %d, %s, %d queries" % (path, name, nq)
            with _Options(g, filter_path=path):
                ids, sc, _, info = g.search_filtered(prob.queries(0, nq), prob.k, allow)
            assert info["allowed"] == int(allow.sum()) and (path == 0 or info["path"] == path), (what, info)
            _same_topk(ids, sc, want, what)
            print("\n%s: %s" % (what, info))
    _stats(g, "filter_path %d" % path)


@pytest.mark.parametrize("form", [0, 1])
def test_range_search(case, form):
    """min_score = the lowest victim's exact score: its 16-bit score lies 0.96 ... 0.997 of eps below it; one unit higher the
    victims of the lowest level leave, and nothing else"""
    g, prob = case
    g.status(reset=True)
    for up in (0, 1):
        ms = prob.range_min_score(form, up)
        for nq in (prob.patterns, 70):
            wl, wi, ws = prob.range_truth(ms, form, nq)
            lims, ids, sc, _ = g.range_search(prob.queries(form, nq), ms)
            what = "query form %d, threshold + %d units, %d queries" % (form, up, nq)
            assert lims.dtype == np.int64 and ids.dtype == np.int64 and sc.dtype == np.float32
            if not np.array_equal(lims, wl):
                q = int(np.flatnonzero(np.diff(lims) != np.diff(wl))[0])
                raise AssertionError("%s: query %d has %d hits, the truth has %d" % (what, q, np.diff(lims)[q], np.diff(wl)[q]))
            assert np.array_equal(ids, wi), what
            assert np.array_equal(sc.view(np.uint32), ws.astype(np.float32).view(np.uint32)), "%s: score bits differ" % what
    st = g.status(reset=True)
    assert st["overflow_batches"] == 0, st
    _stored(g, prob)
