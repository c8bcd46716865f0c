"""GPU: mining.hard_negatives_hip against a numpy restatement of the selection loop of the reference's create_epoch_tuples
(src/datasets/traindataset.py:219-247; tests/_grouped_truth.py: reference_negatives) fed the library's own full ranking of the pool."""
import numpy as np
import pytest

import _grouped_truth as gt

pytestmark = pytest.mark.gpu

P, Q, D = 600, 20, 64


@pytest.fixture(scope="module")
def pool():
    """P pool images in clusters of 1 .. 40, Q queries, each a noisy copy of the centre of a cluster of its own: that cluster's
    images are the nearest of the pool.  Columns are unit vectors, as the reference's descriptors are.  -> qvecs [D, Q], poolvecs
    [D, P], pool clusters, query clusters, ranks [P, Q] from the library's own full ranking"""
    from isehr_amd import _lib
    rng = np.random.default_rng(600)
    sizes = []
    while sum(sizes) < P:
        sizes.append(int(min(1 + rng.integers(0, 40) ** 2 // 40, P - sum(sizes))))    # 1 .. 40, small clusters more often
    assert len(sizes) >= 36 and min(sizes) == 1 and max(sizes) >= 35                  # more clusters than the largest nnum
    clusters = np.repeat(np.arange(len(sizes)) * 3 + 1, sizes)           # ids that are not dense
    centres = rng.standard_normal((len(sizes), D))
    pv = centres[np.repeat(np.arange(len(sizes)), sizes)] + 0.3 * rng.standard_normal((P, D))
    perm = rng.permutation(P)
    pv, clusters = pv[perm], clusters[perm]
    own = rng.choice(len(sizes), Q, replace=False)
    qv = centres[own] + 0.1 * rng.standard_normal((Q, D))
    pv = (pv / np.linalg.norm(pv, axis=1, keepdims=True)).astype(np.float32)
    qv = (qv / np.linalg.norm(qv, axis=1, keepdims=True)).astype(np.float32)
    qclusters = own * 3 + 1
    with _lib.Gallery.from_host(pv, norm_mode=_lib.NORM_NONE) as g:
        ranks = g.search(qv, P)[0].T
    assert (clusters[ranks[0]] == qclusters).all()                        # every query's own cluster is planted nearest
    return np.ascontiguousarray(qv.T), np.ascontiguousarray(pv.T), clusters, qclusters, ranks


def _avg(qv, pv, nidxs):
    total, cnt = 0.0, 0
    for q in range(nidxs.shape[0]):
        for p in nidxs[q]:
            if p >= 0:
                total += float(np.sqrt(((qv[:, q].astype(np.float64) - pv[:, p].astype(np.float64) + 1e-6) ** 2).sum()))
                cnt += 1
    return total / cnt


@pytest.mark.parametrize("nnum", [5, 30])
def test_hard_negatives(pool, nnum):
    from isehr_amd import mining
    qv, pv, clusters, qclusters, ranks = pool
    want = gt.reference_negatives(ranks, clusters, qclusters, nnum)
    assert (want >= 0).all()
    nidxs, avg = mining.hard_negatives_hip(qv, pv, clusters, qclusters, nnum)
    assert nidxs.dtype == np.int64 and nidxs.shape == (Q, nnum) and np.array_equal(nidxs, want)
    assert (clusters[nidxs] != qclusters[:, None]).all()
    assert all(len(set(clusters[row].tolist())) == nnum for row in nidxs)
    ref = _avg(qv, pv, want)
    assert abs(avg - ref) <= 1e-12 * ref
    import torch
    same = mining.hard_negatives_hip(torch.from_numpy(qv), torch.from_numpy(pv), clusters.tolist(), qclusters.tolist(), nnum)
    assert np.array_equal(same[0], nidxs) and same[1] == avg


def test_short_of_clusters_is_padded(pool):
    """the reference raises IndexError when a query runs out of clusters; here the row is padded with -1"""
    from isehr_amd import mining
    qv, pv, clusters, qclusters, ranks = pool
    few = clusters % 4                                                    # at most four clusters in the pool
    qfew = qclusters % 4
    have = len(set(few.tolist()))
    want = gt.reference_negatives(ranks, few, qfew, 5)
    assert ((want >= 0).sum(axis=1) == have - 1).all() and have - 1 < 5
    nidxs, avg = mining.hard_negatives_hip(qv, pv, few, qfew, 5)
    assert np.array_equal(nidxs, want) and (nidxs[:, have - 1:] == -1).all()
    ref = _avg(qv, pv, want)
    assert abs(avg - ref) <= 1e-12 * ref
