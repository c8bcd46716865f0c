"""CPU: pins tests/_kr_truth.py (the sparse, staged restatement of k-reciprocal re-ranking) to oracle.kr_reranking and to the
reference's captured output, and proves what tests/test_gpu_kr_rerank_edges.py relies on: the integer form of the 2/3 rule, that
its k2 = 1 cases tell float32 V from float16 V, and that at most 1 % of any case's entries sit on a float16 rounding boundary."""
import os

import numpy as np
import pytest

import oracle
from isehr_amd.synth import synth_rows

import _kr_truth as T


def _clustered(seed, n, d, ncl, nq, step):                  # the inputs of tests/test_gpu_kr_rerank.py and oracle/make_golden.py
    v = synth_rows(seed, 0, n, d).astype(np.float64)
    c = synth_rows(seed + 1, 0, ncl, d).astype(np.float64)
    v = 0.6 * v + 1.3 * c[np.arange(n) % ncl]
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    q = v[::step][:nq] + 0.15 * synth_rows(seed + 2, 0, nq, d)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return q.T.astype(np.float32), v.T.astype(np.float32)


def test_truth_is_the_oracle_bit_for_bit_on_the_golden_case(golden_dir):
    qv, vecs = _clustered(98, 400, 32, 25, 7, 57)
    t = T.kr_truth(qv, vecs)
    idx, final = oracle.kr_reranking(qv, vecs, return_dist=True)
    assert t.final.dtype == final.dtype == np.float32
    assert np.array_equal(t.final, final) and np.array_equal(t.order, idx)
    assert np.array_equal(t.order, np.load(os.path.join(golden_dir, "kr_rerank.npz"))["indices"])


@pytest.mark.parametrize("name", ["k2_1-k1_5-lam_0.3", "k2_is_k1+1", "all_257"])
def test_truth_is_the_oracle_bit_for_bit(name):
    qv, vecs, k1, k2, lam, t = T.case(name)
    idx, final = oracle.kr_reranking(qv, vecs, k1=k1, k2=k2, lambda_value=lam, return_dist=True)
    assert np.array_equal(t.final, final) and np.array_equal(t.order, idx)


def test_truth_stages_are_consistent():
    qv, vecs, k1, k2, lam, t = T.case("k2_is_k1+1")
    n_all = qv.shape[1] + vecs.shape[1]
    assert t.S.shape == (n_all, n_all) and t.initial_rank.shape == (n_all, k1 + 1)
    assert (t.initial_rank[:, 0] == np.arange(n_all)).all()                  # no duplicates: every image is its own nearest
    for i in (0, 5, n_all - 1):
        assert (np.diff(t.R[i]) > 0).all() and i in t.R[i]
        assert t.V[i].dtype == np.float32 and abs(float(t.V[i].sum()) - 1) < 1e-6
        assert t.Vqe_vals[i].dtype == np.float16 and (np.diff(t.Vqe_cols[i]) > 0).all()
    assert np.allclose(t.dmax, (2 - 2 * t.S).max(axis=1), atol=1e-6)
    assert T.case("k2_1-k1_5-lam_0")[5].Vqe_vals[0].dtype == np.float32      # k2 == 1: V as it is


def test_stable_smallest_is_a_stable_argsort():
    rng = np.random.default_rng(0)
    for n in (2049, 3000, 4112):                            # above the size sorted whole; 16 | 4112
        d = (rng.integers(0, 300, (n, 37)).astype(np.float32) / 7).T          # many ties, a transposed view like the caller's
        for k in (1, 6, 21, 64):
            assert np.array_equal(T.stable_smallest(d, k), np.argsort(d, axis=1, kind="stable")[:, :k])


def test_near_f16_boundary():
    h = np.float16(0.0123)
    up = np.nextafter(h, np.float16(1))
    mid = (np.float64(h) + np.float64(up)) / 2
    vals = np.array([h, up, mid * (1 + 5e-7), mid * (1 - 5e-7), mid * (1 + 4e-6), mid * (1 - 4e-6)], dtype=np.float32)
    assert T.near_f16_boundary(vals).tolist() == [False, False, True, True, False, False]


def test_integer_two_thirds_rule_is_the_float_rule():
    """kr_sets_kernel's `inter * 3 > 2 * ncs` against `len(intersect1d) > 2. / 3 * len(candidate)` (:568), all sizes a wave holds."""
    for ncs in range(0, 65):
        for inter in range(0, ncs + 1):
            assert (inter * 3 > 2 * ncs) == (inter > 2. / 3 * ncs), (inter, ncs)


@pytest.mark.parametrize("name", T.K2_ONE)
def test_k2_one_cases_tell_float32_from_float16(name):
    """Rounding V through float16 at k2 = 1 (what the kernels did before) moves some final distance by ten times the GPU
    test's tolerance or more: that test fails on such a kernel."""
    qv, vecs, k1, k2, lam, t = T.case(name)
    assert k2 == 1 and not t.exposed.any()
    h = T.kr_truth(qv, vecs, k1, k2, lam, force_f16=True)
    moved = float(np.abs(h.final.astype(np.float64) - t.final).max())
    print("float16 V moves the final distance by %.3g" % moved)
    assert moved >= 10 * T.TOL


def test_duplicates_case_has_rows_outside_their_own_neighbour_list():
    qv, vecs, k1, k2, lam, t = T.case("duplicates")
    nq = qv.shape[1]
    same = np.flatnonzero((vecs.T == vecs.T[3]).all(axis=1)) + nq
    group = np.concatenate([[0], same])                                      # query 0 equals the image too
    assert len(same) == 9 and (qv.T[0] == vecs.T[3]).all()
    s = t.S[np.ix_(group, group)]
    assert (s == s[0, 0]).all()                                              # exact ties under the float64-rounded S
    assert (t.initial_rank[group] == group[:k1 + 1]).all()                   # the lower-index rule
    missing = [i for i in group if i not in t.initial_rank[i]]
    assert len(missing) == len(group) - (k1 + 1) == 4
    # at k2 = 1 the row of such an image is its own V row, not that of initial_rank[i, 0]
    t1 = T.case("duplicates-k2_1")[5]
    i = missing[0]
    assert not np.array_equal(t1.Vqe_cols[i], t1.Vqe_cols[int(t1.initial_rank[i, 0])])


@pytest.mark.parametrize("name", list(T.CASES))
def test_exposed_share_of_every_gpu_case(name):
    t = T.case(name)[5]
    share = float(t.exposed.mean())
    print("%s: exposed share %.5f" % (name, share))
    assert share <= 0.01
    if T.CASES[name][7] == 1:
        assert share == 0
