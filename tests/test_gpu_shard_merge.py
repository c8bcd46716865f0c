"""GPU: the shard merge (merge_kernel<true|false>, csrc/select.hip) and the K-th largest of the gathered approximate scores
(kth_of_gathered_kernel -> block_kth_largest) on their own, bit for bit against tests/_shard_aux_truth.py.

Merge: out_idx equals merge_truth, out_score equals it as uint32 with NaN == NaN, at sizes on both sides of the 48 KiB LDS
limit (3072 entries) up to the 8192-entry limit, for full lists of distinct scores, three-valued scores whose ties are decided
by id across the lists, short and empty lists, and +-inf / +-0.0 / out-of-float32-range / NaN scores -- through both entry
points, the packed [score | index] layout of sharded.py, a stride with a poisoned gap, and without out_score.  The outputs
are pre-filled with a sentinel.

K-th: the bit pattern equals kth_truth at n = nshards * k around the 256-thread trips of the radix select, for keys that agree
in all but one byte, all-equal keys, +-x, +-0.0, denormals, a -inf K-th, NaN entries and waves holding eight digits at once.

The only conditional comparison is 'expected NaN => require NaN' (counted in tests/test_shard_aux_truth_cpu.py).

Every case passed on the parent commit's kernels: the kernels are unchanged, the commit adds argument checks only."""
import numpy as np
import pytest

import _shard_aux_truth as T

pytestmark = pytest.mark.gpu

IDX_SENTINEL = -7777
SCORE_SENTINEL = 12345.0


@pytest.fixture(scope="module")
def lib():
    from isehr_amd import _lib
    _lib.load()
    return _lib


def _dev(a):
    """Host array -> device tensor of the same bytes (through an integer view: NaN payloads and -0.0 travel untouched)."""
    import torch
    a = np.ascontiguousarray(a)
    view = {4: np.int32, 8: np.int64}[a.dtype.itemsize]
    return torch.from_numpy(a.view(view).copy()).to(torch.device("cuda", 0))


def _same_scores(got, want):
    g, w = got.view(np.uint32), want.view(np.uint32)
    nan = np.isnan(want)
    return bool(np.all(np.isnan(got[nan])) and np.array_equal(g[~nan], w[~nan]))


def _outputs(nq, k):
    import torch
    dev = torch.device("cuda", 0)
    oi = torch.full((nq, k), IDX_SENTINEL, dtype=torch.int64, device=dev)
    osc = torch.full((nq, k), SCORE_SENTINEL, dtype=torch.float32, device=dev)
    return oi, osc


@pytest.mark.parametrize("kind", T.MERGE_KINDS)
@pytest.mark.parametrize("nq", T.MERGE_NQ)
@pytest.mark.parametrize("nshards,k", T.MERGE_SIZES)
def test_merge_equals_the_truth(lib, nshards, k, nq, kind):
    import torch
    stream = torch.cuda.current_stream().cuda_stream
    s, i, _ = T.sorted_shard_lists(kind, nshards, nq, k)
    want_i, want_s = T.merge_truth(s, i, k)
    per = nq * k

    def check(tag, oi, osc):
        torch.cuda.synchronize()
        got_i = oi.cpu().numpy()
        assert np.array_equal(got_i, want_i), "%s: first difference at %s" % (tag, np.argwhere(got_i != want_i)[:3].tolist())
        if osc is not None:
            got_s = osc.cpu().numpy()
            assert _same_scores(got_s, want_s), tag

    # contiguous [S][Q][k]
    sd, idd = _dev(s), _dev(i)
    oi, osc = _outputs(nq, k)
    lib.topk_merge_device(sd.data_ptr(), idd.data_ptr(), nshards, nq, k, oi.data_ptr(), osc.data_ptr(), stream)
    check("contiguous", oi, osc)
    # without scores
    oi, osc = _outputs(nq, k)
    lib.topk_merge_device(sd.data_ptr(), idd.data_ptr(), nshards, nq, k, oi.data_ptr(), None, stream)
    check("no out_score", oi, None)
    torch.cuda.synchronize()
    assert np.all(osc.cpu().numpy() == np.float32(SCORE_SENTINEL))
    # the packed [S][2][Q][k] buffer of the sharded search: scores, then indices, shard stride 2 * nq * k
    pack = np.empty((nshards, 2, per), dtype=np.int64)
    pack[:, 0] = s.reshape(nshards, per).view(np.int64)
    pack[:, 1] = i.reshape(nshards, per)
    pd = _dev(pack)
    oi, osc = _outputs(nq, k)
    lib.topk_merge_strided_device(pd[0, 0].data_ptr(), pd[0, 1].data_ptr(), 2 * per, nshards, nq, k, oi.data_ptr(),
                                  osc.data_ptr(), stream)
    check("packed", oi, osc)
    # a stride with a gap: +inf scores with plausible ids lie in it
    gap = 5
    sg = np.full((nshards, per + gap), np.inf, dtype=np.float64)
    ig = np.full((nshards, per + gap), 1 << 40, dtype=np.int64)
    sg[:, :per], ig[:, :per] = s.reshape(nshards, per), i.reshape(nshards, per)
    sgd, igd = _dev(sg), _dev(ig)
    oi, osc = _outputs(nq, k)
    lib.topk_merge_strided_device(sgd.data_ptr(), igd.data_ptr(), per + gap, nshards, nq, k, oi.data_ptr(), osc.data_ptr(),
                                  stream)
    check("gap", oi, osc)


def test_single_shard_merge_is_a_copy(lib):
    import torch
    stream = torch.cuda.current_stream().cuda_stream
    s, i, _ = T.sorted_shard_lists("special", 1, 5, 100)
    oi, osc = _outputs(5, 100)
    sd, idd = _dev(s), _dev(i)
    lib.topk_merge_device(sd.data_ptr(), idd.data_ptr(), 1, 5, 100, oi.data_ptr(), osc.data_ptr(), stream)
    torch.cuda.synchronize()
    assert np.array_equal(oi.cpu().numpy(), i[0])
    with np.errstate(over="ignore"):
        want = np.where(i[0] >= 0, s[0], -np.inf).astype(np.float32)
    assert _same_scores(osc.cpu().numpy(), want)


@pytest.mark.parametrize("first_kind", range(len(T.KTH_KINDS)), ids=T.KTH_KINDS)
@pytest.mark.parametrize("nshards,k", T.KTH_SIZES)
def test_kth_of_gathered_equals_the_truth(lib, nshards, k, first_kind):
    import torch
    stream = torch.cuda.current_stream().cuda_stream
    g, _ = T.kth_inputs(first_kind, nshards, k)
    want = T.kth_truth(g, k)
    out = torch.full((T.KTH_NQ,), SCORE_SENTINEL, dtype=torch.float32, device=torch.device("cuda", 0))
    gd = _dev(g)
    lib.kth_of_gathered_device(gd.data_ptr(), nshards, T.KTH_NQ, k, out.data_ptr(), stream)
    torch.cuda.synchronize()
    got = out.view(torch.int32).cpu().numpy().view(np.uint32)
    nan = np.isnan(want.view(np.float32))
    kinds = [T.KTH_KINDS[(first_kind + q) % len(T.KTH_KINDS)] for q in range(T.KTH_NQ)]
    assert np.all(np.isnan(got.view(np.float32)[nan])), (kinds, got, want)
    assert np.array_equal(got[~nan], want[~nan]), (kinds, ["%08x" % v for v in got], ["%08x" % v for v in want])
