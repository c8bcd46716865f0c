"""GPU: the sharded protocol's worst-shard margin (mi_knn_phase1_device, the gathered K-th score, mi_knn_phase2_device, the merge;
DESIGN 7) on data that attains the rounding bound across shards, all three shards on one GPU.

tests/_margin_truth_sharded.py lays the victims and imposters of tests/_margin_truth.py out over three contiguous shards.  A
split pattern has its K imposters on one shard and its K victims on another: the victims are found only if their shard cuts at
the GATHERED L with the whole margin (0.95 ... 0.985 of it is needed).  A quiet pattern has its victims on a shard whose own
max |g^ - g| is a quarter of the imposters' shard's: they lie 2.1 ... 2.35 of that shard's own margin below L and are found only
because the shards agreed on the norm maxima first (ShardedGallery._agree; restated here with norm_bounds(raise_to=...), as
tests/test_gpu_shape_sweep.py::_simulated_shards does).  tests/test_margin_truth_sharded_cpu.py shows that the host model of the
protocol loses a victim for every quiet query without the agreement and for every split query at 0.85 of the margin.  Every score
is exact in every format and order, so ids are compared with == and scores as bits -- the merged answer, every shard's phase-2
list, and the single gallery over the concatenated rows -- and the candidates summed over the shards are the 2 K per query the
model counts."""
import numpy as np
import pytest

import _margin_truth_sharded as ms

pytestmark = pytest.mark.gpu

IDS = ["d%d-%s-n%d" % c[:3] for c in ms.CASES]
NQS = (1, 70, 129, 300)               # the streaming kernel, its last batch size + 1, the tile kernel


@pytest.fixture(scope="module", params=ms.CASES, ids=IDS)
def case(request):
    from isehr_amd import _lib
    from isehr_amd.sharded import shard_bounds
    prob = ms.problem(*request.param)
    f16 = 1 if prob.image == "f16" else 0
    shards = []
    _lib.set_global_option("image_dtype", f16)
    try:
        for r in range(ms.SHARDS):
            lo, hi = shard_bounds(prob.n, ms.SHARDS, r)
            assert (lo, hi) == prob.bounds[r]
            shards.append(_lib.Gallery.from_host(prob.X[lo:hi], norm_mode=_lib.NORM_NONE, row_offset=lo))
        single = _lib.Gallery.from_host(prob.X, norm_mode=_lib.NORM_NONE)
        shards.append(single)
    finally:
        _lib.set_global_option("image_dtype", 1)
    try:
        for r, sh in enumerate(shards[:ms.SHARDS]):
            lo, hi = prob.bounds[r]
            assert int(sh.get_option("image_dtype")) == f16, "shard %d took another image type" % r
            R = sh.get_rows(0, sh.n)
            assert sh.n == hi - lo and np.array_equal(R.view(np.uint32), prob.X[lo:hi].view(np.uint32))
            # the shard's OWN maxima, before the agreement: the quiet shard's max |g^ - g| is about a quarter of a loud one's
            own = np.array(sh.norm_bounds(), np.float32)
            assert np.allclose(own, np.array(prob.shard_norm_bounds(r), np.float32), rtol=4e-7, atol=0), (r, own)
        assert int(single.get_option("image_dtype")) == f16
        # the agreement of ShardedGallery._agree: the image type is the coarsest (asserted equal above), the maxima all-reduced
        agreed = np.max(np.array([sh.norm_bounds() for sh in shards[:ms.SHARDS]]), axis=0)
        for sh in shards[:ms.SHARDS]:
            got = np.array(sh.norm_bounds(raise_to=[float(v) for v in agreed]), np.float32)
            assert np.allclose(got, np.array(prob.agreed_bounds(), np.float32), rtol=4e-7, atol=0)
        yield shards[:ms.SHARDS], single, prob
    finally:
        for sh in shards:
            sh.close()


def _protocol(shards, Q, k):
    """tests/test_gpu_shape_sweep.py::_simulated_shards on shards that exist already (image type and maxima agreed by the
    fixture) -> merged ids, merged float32 scores, per-shard ids [G, nq, k], per-shard float64 scores, flags"""
    import torch
    from isehr_amd import _lib
    G, nq = len(shards), Q.shape[0]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    q = torch.from_numpy(Q).to(dev)
    approx = torch.empty((G, nq, k), dtype=torch.float32, device=dev)
    for r, sh in enumerate(shards):
        sh.phase1_device(q.data_ptr(), nq, k, approx[r].data_ptr(), stream)
    L = torch.empty((nq,), dtype=torch.float32, device=dev)
    _lib.kth_of_gathered_device(approx.data_ptr(), G, nq, k, L.data_ptr(), stream)
    idx = torch.empty((G, nq, k), dtype=torch.int64, device=dev)
    sc = torch.empty((G, nq, k), dtype=torch.float32, device=dev)
    sc64 = torch.empty((G, nq, k), dtype=torch.float64, device=dev)
    for r, sh in enumerate(shards):
        sh.phase2_device(nq, k, L.data_ptr(), idx[r].data_ptr(), sc[r].data_ptr(), sc64[r].data_ptr(), stream)
    oi = torch.empty((nq, k), dtype=torch.int64, device=dev)
    os_ = torch.empty((nq, k), dtype=torch.float32, device=dev)
    _lib.topk_merge_device(sc64.data_ptr(), idx.data_ptr(), G, nq, k, oi.data_ptr(), os_.data_ptr(), stream)
    torch.cuda.synchronize()
    flags = [sh.flags() for sh in shards]
    return oi.cpu().numpy(), os_.cpu().numpy(), idx.cpu().numpy(), sc64.cpu().numpy(), L.cpu().numpy(), flags


def _same_ids(ids, want, what):
    assert ids.dtype == np.int64 and ids.shape == want.shape
    if not np.array_equal(ids, want):
        q, j = (int(v[0]) for v in np.nonzero(ids != want))
        lost = sorted(set(want[q].tolist()) - set(ids[q].tolist()))
        raise AssertionError("%s: query %d, position %d: row %d, the truth has row %d; %d true rows are missing (first: %s)"
                             % (what, q, j, ids[q, j], want[q, j], len(lost), lost[:5]))


SETTINGS = [("defaults", {}), ("rigorous chunk schedule", {"speculative": 0})]


@pytest.mark.parametrize("name, opts", SETTINGS, ids=[s[0].replace(" ", "_") for s in SETTINGS])
def test_protocol(case, name, opts):
    shards, single, prob = case
    _, _, count, sid, ssc = prob.protocol(1.0)
    assert (count.sum(1) == 2 * prob.k).all()
    old = [{k: sh.get_option(k) for k in opts} for sh in shards]
    try:
        for sh in shards:
            for k, v in opts.items():
                sh.set_option(k, v)
            sh.status(reset=True)
        for nq in NQS:
            what = "%s, %d queries" % (name, nq)
            Q, (wi, ws), pick = prob.queries(0, nq), prob.truth(nq=nq), prob.of_query(nq)
            oi, os_, idx, sc64, L, flags = _protocol(shards, Q, prob.k)
            assert not any(flags), (what, flags)
            assert np.array_equal(L.astype(np.float64), prob.gathered_kth()[pick]), "%s: the gathered K-th score" % what
            _same_ids(oi, wi, what)
            assert os_.dtype == np.float32 and np.array_equal(os_.view(np.uint32), ws.astype(np.float32).view(np.uint32)), \
                "%s: merged score bits differ" % what
            got = 0
            for r, sh in enumerate(shards):
                # what each shard contributed: its rows within the agreed margin of L by (exact score desc, id asc), float64 bits
                _same_ids(idx[r], sid[r][pick], "%s, shard %d" % (what, r))
                assert np.array_equal(sc64[r].view(np.uint64), ssc[r][pick].view(np.uint64)), "%s, shard %d: float64 bits" % (what, r)
                st = sh.status(reset=True)
                assert st["overflow_batches"] == 0 and st["spec_retries"] == 0, (what, r, st)
                print("\n%s, shard %d: survivors %d, candidates %d over %d queries" % (what, r, st["survivors"], st["candidates"], st["queries"]))
                assert st["candidates"] == int(count[pick, r].sum()), (what, r, st)
                got += st["candidates"]
            assert got == 2 * prob.k * nq
            # the single gallery over the concatenated rows: the same ids and bits
            ids1, sc1, _ = single.search(Q, prob.k)
            _same_ids(ids1, oi, what + ", single gallery")
            assert np.array_equal(sc1.view(np.uint32), os_.view(np.uint32)), "%s: single-gallery score bits differ" % what
    finally:
        for sh, o in zip(shards, old):
            for k, v in o.items():
                sh.set_option(k, v)

