"""GPU: k-reciprocal re-ranking (csrc/kr_rerank.hip, mi_kr_rerank) against the staged restatement of tests/_kr_truth.py at the
sizes, constants and inputs its five kernels branch on.  Every case asserts (T.check_result): each row a permutation,
ascending distances, |truth - dist| <= 2e-6 (plus one float16 ulp through the Jaccard slope on the entries the truth marks as
exposed to a float16 rounding boundary), and position by position a different image only where the truth's own distances agree
within that bound.  tests/test_kr_rerank_cpu.py pins the truth to the oracle bit for bit and proves the exposed shares written beside the seeds in T.CASES.

Stages are isolated by their inputs: lambda = 1 leaves dist / dmax alone (kr_weights_kernel's row maximum, the scorer), lambda = 0
the Jaccard pass alone, k2 = 1 takes the float16 rounding and the row mean out of V_qe, k1 = 5 keeps the sets tiny.

On the parent of the commit that made kr_expand_kernel keep V in float32 at k2 = 1 (and take row i itself there), seven of the
17 parametrised cases failed on an MI355X and the other ten passed: the six k2_1 cases with distance errors of 1.04e-4 (k1 = 2 and 5, lambda = 0), 7.3e-5
(k1 = 2 and 5, lambda = 0.3), 4.8e-5 and 3.4e-5 (k1 = 8), and duplicates-k2_1 with 0.70.  With the fix the largest error of any case
is 1.2e-7."""
import numpy as np
import pytest

import _kr_truth as T

pytestmark = pytest.mark.gpu


def _run(name):
    from isehr_amd.reranking import kr_reranking_hip
    qv, vecs, k1, k2, lam, t = T.case(name)
    got, dist = kr_reranking_hip(qv, vecs, k1=k1, k2=k2, lambda_value=lam, return_dist=True)
    return got, dist, t


@pytest.mark.parametrize("name", [n for n in T.CASES if n != "large-lds"])
def test_kr_rerank_edge_case(name):
    got, dist, t = _run(name)
    T.check_result(t, got, dist)


def test_kr_rerank_above_64_kb_of_lds():
    """all = 16503 > 16384 and no multiple of 256: kr_expand_kernel's accumulator row needs the large-LDS opt-in."""
    got, dist, t = _run("large-lds")
    T.check_result(t, got, dist)


def test_kr_rerank_float64_input_is_the_float32_result():
    """kr_pack_kernel<double>: float64 copies of float32 values convert back exactly (torch.tensor(..., dtype=torch.float32))."""
    from isehr_amd.reranking import kr_reranking_hip
    qv, vecs, k1, k2, lam, t = T.case("k2_is_k1+1")
    got, dist = kr_reranking_hip(qv.astype(np.float64), vecs.astype(np.float64), k1=k1, k2=k2, lambda_value=lam, return_dist=True)
    ref, rdist = _run("k2_is_k1+1")[:2]
    assert np.array_equal(got, ref) and np.array_equal(dist, rdist)
    T.check_result(t, got, dist)


def test_kr_rerank_strided_rows_are_the_contiguous_result():
    """Both strides non-unit, for queries and gallery: [::2, ::3] slices of a larger array filled with other values."""
    from isehr_amd import _lib
    qv, vecs, k1, k2, lam, t = T.case("n_700")
    q, g = np.ascontiguousarray(qv.T), np.ascontiguousarray(vecs.T)
    rng = np.random.default_rng(5)
    big_q = rng.standard_normal((2 * q.shape[0], 3 * q.shape[1])).astype(np.float32)
    big_g = rng.standard_normal((2 * g.shape[0], 3 * g.shape[1])).astype(np.float32)
    big_q[::2, ::3], big_g[::2, ::3] = q, g
    sq, sg = big_q[::2, ::3], big_g[::2, ::3]
    assert sq.strides == (2 * big_q.strides[0], 12) and sg.strides == (2 * big_g.strides[0], 12)
    got, dist = _lib.kr_rerank(sq, sg, k1, k2, lam, 0, True)
    ref, rdist = _lib.kr_rerank(q, g, k1, k2, lam, 0, True)
    assert np.array_equal(got, ref) and np.array_equal(dist, rdist)
    T.check_result(t, got, dist)
