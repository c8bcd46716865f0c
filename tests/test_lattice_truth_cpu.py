"""The premises of the exact range-search and filtered top-K tests (tests/_lattice_truth.py), shown on the host: lattice scores
are the same number in float16 products with float32 accumulation, in bfloat16 products with float32 accumulation, in float32
and in float64, under any order of the sum and at every partial sum; the generator delivers the hit counts it is asked for; the
truths are what they say."""
import numpy as np
import pytest

import _lattice_truth as lt


def _orders(rng, d):
    """summation orders over the K dimension: forward, backward, two random"""
    return [np.arange(d), np.arange(d)[::-1].copy(), rng.permutation(d), rng.permutation(d)]


def _partial_sums(prod, acc_dtype):
    """prod [nq, n, d] products -> [nq, n, d] running sums in acc_dtype, added one term after the other"""
    return np.cumsum(prod.astype(acc_dtype), axis=2, dtype=acc_dtype)


def _products(X, Q, how):
    """[nq, n, d] elementwise products computed in the number format `how`, returned as float64 (exact)"""
    if how == "bfloat16":
        import torch
        Xb, Qb = torch.from_numpy(X).to(torch.bfloat16), torch.from_numpy(Q).to(torch.bfloat16)
        assert (Xb.float().numpy() == X).all() and (Qb.float().numpy() == Q).all()
        p = Qb[:, None, :] * Xb[None, :, :]
        assert p.dtype == torch.bfloat16
        return p.float().numpy().astype(np.float64)
    t = np.dtype(how)
    Xt, Qt = X.astype(t), Q.astype(t)
    assert (Xt.astype(np.float64) == X).all() and (Qt.astype(np.float64) == Q).all()
    p = Qt[:, None, :] * Xt[None, :, :]
    assert p.dtype == t
    return p.astype(np.float64)


# (format of the operands and products, format of the accumulator)
FORMATS = [("float16", np.float32), ("float16", np.float16), ("bfloat16", np.float32), ("float32", np.float32),
           ("float64", np.float64)]


def _check_exact(X, Q, want, scale):
    """every format, every order: every partial sum and the score equal the integer arithmetic (scores = want / scale)"""
    rng = np.random.default_rng(5)
    for how, acc in FORMATS:
        for perm in _orders(rng, X.shape[1]):
            prod = _products(X[:, perm], Q[:, perm], how)
            run = _partial_sums(prod, acc)
            exact = np.cumsum(np.rint(prod * scale).astype(np.int64), axis=2)
            assert (np.rint(prod * scale) == prod * scale).all()
            assert (run.astype(np.float64) * scale == exact).all(), (how, acc)
            assert (run[:, :, -1].astype(np.float64) * scale == want).all(), (how, acc)


@pytest.mark.parametrize("d", [1, 32, 100, 128])
def test_integer_lattice_scores_are_exact_in_every_format_and_order(d):
    rng = np.random.default_rng(d)
    X = lt.int_rows(rng, 48, d)
    X[0], X[1] = lt.HI, lt.LO                                  # the extreme rows: |score| reaches 9 d
    Q = np.concatenate([lt.dense_queries(rng, 5, d), np.full((1, d), lt.HI, np.float32)])
    S = lt.int_scores(X, Q)
    assert S.dtype == np.int64 and np.abs(S).max() == 9 * d <= 1152 < 2048
    _check_exact(X, Q, S, 1)
    assert (S.astype(np.float32).astype(np.int64) == S).all() and (S.astype(np.float16).astype(np.int64) == S).all()


def test_unit_lattice_norms_and_scores_are_exact():
    rng = np.random.default_rng(64)
    X = lt.unit_rows(rng, 48)
    Q = lt.unit_rows(rng, 6)
    X[0], X[1] = Q[0], -Q[0]
    S = lt.unit_scores(X, Q)
    assert S[0, 0] == 1.0 and S[0, 1] == -1.0 and np.abs(S).max() == 1.0
    assert (np.rint(S * 32) == S * 32).all()                    # multiples of 1/32
    _check_exact(X, Q, np.rint(S * 64).astype(np.int64), 64)
    # the squared norm is exactly 1 in every format and order, so normalising is the identity
    for A in (X, Q):
        n2 = np.rint(lt.unit_scores(A, A).diagonal() * 64).astype(np.int64)
        assert (n2 == 64).all()
        for t in (np.float32, np.float64):
            for perm in _orders(rng, lt.UNIT_D):
                sq = np.cumsum((A[:, perm].astype(t) ** 2), axis=1, dtype=t)[:, -1]
                assert (sq == 1).all() and (np.sqrt(sq) == 1).all()
                assert ((A.astype(t) / np.sqrt(sq)[:, None]) == A).all()
                assert ((A.astype(t) * (1 / np.sqrt(sq))[:, None]) == A).all()


@pytest.mark.parametrize("tau, scale", [(1, 1), (0, 1), (-2, 2), (3, 3), (3, 1)])
def test_generator_delivers_the_requested_hit_counts(tau, scale):
    rng = np.random.default_rng(11)
    n, d = lt.BOUNDARY_N, 32
    counts = lt.BOUNDARY_COUNTS
    L = tau // scale
    if L == lt.HI:                                             # no level above tau: every hit scores exactly tau
        counts = [(a, a) for a, _ in counts]
    X, Q = lt.planted_gallery(rng, n, d, tau, counts, scale)
    assert X.dtype == np.float32 and X.shape == (n, d) and X.min() >= lt.LO and X.max() <= lt.HI
    assert (X == np.rint(X)).all()
    S = lt.int_scores(X, Q)
    assert ((S >= tau).sum(1) == [a for a, _ in counts]).all()
    assert ((S == tau).sum(1) == [b for _, b in counts]).all()
    lims, ids, sc = lt.range_truth(S, tau)
    assert (np.diff(lims) == [a for a, _ in counts]).all()
    assert {2047, 2048, 2049, 4096, 4097} <= set(np.diff(lims).tolist())


def test_generator_small_shapes():
    rng = np.random.default_rng(12)
    for n, d, counts in [(1, 1, [(1, 1)]), (1, 1, [(0, 0)]), (255, 32, [(0, 0), (255, 100), (7, 7)]),
                         (257, 100, [(257, 0), (256, 255)])]:
        X, Q = lt.planted_gallery(rng, n, d, 1, counts)
        S = lt.int_scores(X, Q)
        assert ((S >= 1).sum(1) == [a for a, _ in counts]).all() and ((S == 1).sum(1) == [b for _, b in counts]).all()


def test_range_truth():
    S = np.array([[2, 5, 2, -1, 5, 0], [0, 0, 0, 0, 0, 0], [-3, -3, -3, -3, -3, -3]], np.int64)
    lims, ids, sc = lt.range_truth(S, 0)
    assert lims.tolist() == [0, 5, 11, 11] and lims.dtype == np.int64
    assert ids.tolist() == [1, 4, 0, 2, 5, 0, 1, 2, 3, 4, 5] and ids.dtype == np.int64
    assert sc.tolist() == [5, 5, 2, 2, 0, 0, 0, 0, 0, 0, 0] and sc.dtype == np.float32
    assert lt.range_truth(S, -0.0)[1].tolist() == ids.tolist()
    assert lt.range_truth(S, np.nextafter(0.0, np.inf))[0].tolist() == [0, 4, 4, 4]
    assert lt.range_truth(S, np.nextafter(0.0, -np.inf))[0].tolist() == lims.tolist()
    assert lt.range_truth(S, np.inf)[0].tolist() == [0, 0, 0, 0] and len(lt.range_truth(S, np.inf)[1]) == 0
    assert lt.range_truth(S, -np.inf)[0].tolist() == [0, 6, 12, 18]
    # the order is np.lexsort((ids, -S)) of the members
    rng = np.random.default_rng(3)
    R = rng.integers(-4, 5, size=(4, 300))
    lims, ids, sc = lt.range_truth(R, 1)
    for i in range(4):
        order = np.lexsort((np.arange(300), -R[i]))
        want = order[R[i][order] >= 1]
        assert (ids[lims[i]:lims[i + 1]] == want).all() and (sc[lims[i]:lims[i + 1]] == R[i][want]).all()


def test_filtered_truth():
    S = np.array([[2, 5, 2, -1, 5, 0]], np.int64)
    mask = np.array([0, 0, 1, 1, 1, 1], bool)
    ids, sc = lt.filtered_truth(S, mask, 3, row_offset=100)
    assert ids.tolist() == [[104, 102, 105]] and sc.tolist() == [[5, 2, 0]]
    assert ids.dtype == np.int64 and sc.dtype == np.float32
    ids, sc = lt.filtered_truth(S, mask, 6)
    assert ids.tolist() == [[4, 2, 5, 3, -1, -1]] and sc[0, :4].tolist() == [5, 2, 0, -1] and np.isneginf(sc[0, 4:]).all()
    ids, sc = lt.filtered_truth(S, np.zeros(6, bool), 2)
    assert (ids == -1).all() and np.isneginf(sc).all()
    # ties at k: the lower allowed ids of the class, never a disallowed row
    T = np.array([[1, 1, 1, 1, 1, 1]], np.int64)
    assert lt.filtered_truth(T, mask, 2)[0].tolist() == [[2, 3]]
