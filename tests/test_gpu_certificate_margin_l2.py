"""GPU: the certificate's margin on squared-L2 galleries (mi_knn_search_l2, mi_knn_search_l2_device and the filtered paths; DESIGN
5.11) on data that attains the row term of the augmented bound as far as it can be attained.

tests/_margin_truth_l2.py plants, per query, K victims whose 16-bit score underestimates the exact key s = q.g - 1/2 |g|^2 by
|q^||g^ - g| and K imposters whose 16-bit score overestimates it by as much: the 16-bit top-K is the imposters, the nearest K rows
are the victims, and the lowest victim lies 0.88 ... 0.98 of the shipped margin below the K-th 16-bit score, wherever in its
summation-order band the device's score falls.  tests/test_margin_truth_l2_cpu.py shows that a filter applying 0.85 of the margin
loses a victim for every query at both ends of that band, and that no row lies near enough to a cut for the band to change the
candidate count.  Distances are exact integers in units of (ulp / 64)^2, so ids are compared with ==, dist64 as bits and dist as
float32(dist64) bit for bit; the statistics show that the 16-bit path gave the answer (no overflowed batch, no speculative retry,
exactly the 2 K candidates per query the model counts).

The norm maxima the margin is made of are read from the saved gallery file (norm_bounds() is refused on an L2 gallery: it is the
sharded search's) and must lie within 4e-7 of the model's maxima over the AUGMENTED rows: a maximum that left the hidden columns
out would be 14 % or more off.  fp16 galleries are created with capacity = n, bf16 ones with capacity > n (an appendable L2 gallery
is bf16 from the start): no global option is involved."""
import os
import tempfile

import numpy as np
import pytest

import _gallery_file as gf
import _margin_truth_l2 as ml

pytestmark = pytest.mark.gpu

IDS = ["d%d-%s" % c[:2] for c in ml.CASES]
NQS = (1, 70, 128, 129, 300)


@pytest.fixture(scope="module", params=ml.CASES, ids=IDS)
def case(request):
    from isehr_amd import _lib
    prob = ml.problem(*request.param)
    g = _lib.Gallery.l2_from_host(prob.X, capacity=0 if prob.f16 else prob.n + 256)
    try:
        assert int(g.get_option("image_dtype")) == int(prob.f16), "the gallery took another image type"
        assert g.get_option("metric") == 1 and g.d == prob.d
        _stored(g, prob)
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "l2.gal")
            g.save(path)
            f = gf.read_gallery_file(path)
        assert f.metric == gf.METRIC_L2 and f.ud == prob.d and f.dp == prob.dp and f.img_f16 == int(prob.f16)
        assert np.array_equal(np.ascontiguousarray(f.rows_f32[:, prob.d:prob.d + 3]).view(np.uint32), prob.hidden.view(np.uint32))
        bounds = np.array(f.gstat3, np.float32)
        # the maxima the margin is made of: each within its 1e-6 inflation of the model's (summation order only)
        assert np.allclose(bounds, np.array(prob.aug_bounds(), np.float32), rtol=4e-7, atol=0), (bounds, prob.aug_bounds())
        yield g, prob
    finally:
        g.close()


def _stored(g, prob):
    R = g.get_rows(0, g.n)
    assert g.n == prob.n and np.array_equal(R.view(np.uint32), prob.X.view(np.uint32)), "the gallery does not hold the rows it was given"


def _same(got, want, what):
    ids, dist, dist64 = got[0], got[1], got[2]
    wi, wd = want
    assert ids.dtype == np.int64 and ids.shape == wi.shape
    if not np.array_equal(ids, wi):
        q, j = (int(v[0]) for v in np.nonzero(ids != wi))
        lost = sorted(set(wi[q].tolist()) - set(ids[q].tolist()))
        raise AssertionError("%s: query %d, position %d: row %d, the truth has row %d; %d true rows are missing (first: %s)"
                             % (what, q, j, ids[q, j], wi[q, j], len(lost), lost[:5]))
    assert dist64.dtype == np.float64 and np.array_equal(dist64.view(np.uint64), wd.view(np.uint64)), "%s: dist64 bits differ" % what
    assert dist.dtype == np.float32 and np.array_equal(dist.view(np.uint32), dist64.astype(np.float32).view(np.uint32)), \
        "%s: dist is not float32(dist64)" % what


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
def test_search_l2(case, name, opts):
    g, prob = case
    g.status(reset=True)
    for nq in NQS:
        Q, want = prob.queries(nq), prob.truth(nq=nq)
        what = "%s, %d queries" % (name, nq)
        with _Options(g, **opts):
            got = g.search_l2(Q, prob.k)
        _same(got, want, what)
        _stats(g, what, nq, prob)
    assert (prob.candidates() == 2 * prob.k).all()


def test_force_exact_gives_the_same_bits(case):
    g, prob = case
    for nq in (1, 129):
        Q, want = prob.queries(nq), prob.truth(nq=nq)
        a = g.search_l2(Q, prob.k)
        with _Options(g, force_exact=1):
            b = g.search_l2(Q, prob.k)
        _same(a, want, "16-bit path, %d queries" % nq)
        _same(b, want, "force_exact, %d queries" % nq)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[2].view(np.uint64), b[2].view(np.uint64))
    _stored(g, prob)


@pytest.mark.parametrize("nq", [1, 70])
def test_search_l2_device(case, nq):
    import torch
    g, prob = case
    want = prob.truth(nq=nq)
    g.status(reset=True)
    q = torch.from_numpy(prob.queries(nq)).cuda()
    ix = torch.full((nq, prob.k), -7, dtype=torch.int64, device="cuda")
    d32 = torch.zeros((nq, prob.k), dtype=torch.float32, device="cuda")
    d64 = torch.zeros((nq, prob.k), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    g.search_l2_device(q.data_ptr(), nq, prob.k, ix.data_ptr(), d32.data_ptr(), d64.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert g.flags() == 0
    _same((ix.cpu().numpy(), d32.cpu().numpy(), d64.cpu().numpy()), want, "search_l2_device, %d queries" % nq)
    _stats(g, "search_l2_device, %d queries" % nq, nq, prob)


@pytest.mark.parametrize("path", [1, 2])
def test_search_l2_filtered(case, path):
    """path 1 scores a sub-gallery of the allowed rows under the parent's norm maxima, path 2 over-fetches from the whole gallery"""
    g, prob = case
    g.status(reset=True)
    for name, allow in prob.allow_sets().items():
        for nq in (prob.patterns, 130):
            want = prob.truth(allow=allow, nq=nq)
            what = "filter_path %d, %s, %d queries" % (path, name, nq)
            with _Options(g, filter_path=path):
                got = g.search_l2(prob.queries(nq), prob.k, allow=allow)
            assert got[3]["allowed"] == int(allow.sum()) and got[3]["path"] == path, (what, got[3])
            _same(got, want, what)
            print("\n%s: %s" % (what, got[3]))
    _stats(g, "filter_path %d" % path)
