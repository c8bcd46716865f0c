"""Lattice data and plain numpy truths for the exact range-search and filtered top-K tests.

Every score of the data made here is exactly representable in fp16, bf16, f32 and f64 whatever the order of the sum, so the
host truth is the device's answer to the bit: members by `>=`, order by (score desc, row asc), scores compared as bits.

  integer lattice (NORM_NONE galleries)  rows and queries float32 with integer entries in [-3, 3], d <= 128: every product is an
                                         integer of magnitude <= 9 and every partial sum one of magnitude <= 9 * 128 = 1152 < 2048
                                         (fp16 holds every integer up to 2048, bf16 products are exact and the sums run in f32).
  unit lattice (NORM_L2 galleries)       d = 64, entries +-0.125: the squared norm is 64 / 64 = 1 exactly (normalising is the
                                         identity), every product is +-1/64 and every score a multiple of 1/32 in [-1, 1].

test_lattice_truth_cpu.py proves these premises; the GPU tests assert that the gallery stores the rows bit for bit."""
import numpy as np

LO, HI = -3, 3                 # the integer lattice's entries
D_MAX = 128                    # 9 * 128 = 1152 < 2048
UNIT_D = 64
UNIT = 0.125
RANGE_RUN = 2048               # csrc/csr_order.hip (CSR_RUN): the hits of a query are sorted in runs of this length, then merged
# (rows scoring >= tau, rows scoring == tau) per planted query of a gallery of BOUNDARY_N rows: hit counts on and either side of
# one run and of two runs, with tie classes that reach across positions 2048 and 4096
BOUNDARY_N = 4200
BOUNDARY_COUNTS = [(0, 0), (1, 1), (2047, 700), (2048, 700), (2049, 700), (4096, 1400), (4097, 1400), (4200, 1400)]


def int_scores(X, Q):
    """[nq, n] int64 scores of integer-lattice rows X [n, d] and queries Q [nq, d]"""
    Xi, Qi = X.astype(np.int64), Q.astype(np.int64)
    assert (Xi == X).all() and (Qi == Q).all()
    return Qi @ Xi.T


def unit_scores(X, Q):
    """[nq, n] float64 scores of unit-lattice rows and queries: (signs . signs) / 64, exact"""
    Xs, Qs = (X / UNIT).astype(np.int64), (Q / UNIT).astype(np.int64)
    assert (np.abs(Xs) == 1).all() and (np.abs(Qs) == 1).all() and X.shape[1] == UNIT_D
    return (Qs @ Xs.T).astype(np.float64) / 64.0


def int_rows(rng, n, d):
    assert 1 <= d <= D_MAX
    return rng.integers(LO, HI + 1, size=(n, d)).astype(np.float32)


def dense_queries(rng, nq, d):
    """integer-lattice queries with every coordinate non-zero"""
    mag = rng.integers(1, HI + 1, size=(nq, d))
    return (mag * rng.choice([-1, 1], size=(nq, d))).astype(np.float32)


def unit_rows(rng, n):
    return (UNIT * rng.choice([-1.0, 1.0], size=(n, UNIT_D))).astype(np.float32)


def _spread(count, levels):
    """`count` values spread level by level over `levels` (as evenly as it goes, the first levels take the remainder)"""
    if count == 0:
        return np.zeros(0, np.int64)
    assert len(levels) > 0, "no level left for %d rows" % count
    each, rest = divmod(count, len(levels))
    return np.concatenate([np.full(each + (1 if i < rest else 0), lv, np.int64) for i, lv in enumerate(levels)])


def planted_gallery(rng, n, d, tau, counts, scale=1):
    """Integer-lattice gallery [n, d] and one-hot queries [len(counts), d] with controlled hit counts at the integer threshold
    `tau`: query i is `scale * e_i`, so its score is scale * X[:, i], and column i is filled level by level so that exactly
    counts[i][0] rows score >= tau and exactly counts[i][1] of them score == tau; the levels above and below tau share the other
    rows evenly (large tie classes), the rows of every level are placed at random and the other columns are random lattice
    values.  tau must be a multiple of scale."""
    assert 1 <= scale <= HI and tau % scale == 0 and len(counts) <= d
    L = tau // scale
    assert LO <= L <= HI
    X = int_rows(rng, n, d)
    Q = np.zeros((len(counts), d), np.float32)
    for i, (n_ge, n_eq) in enumerate(counts):
        assert 0 <= n_eq <= n_ge <= n
        col = np.concatenate([np.full(n_eq, L, np.int64), _spread(n_ge - n_eq, list(range(L + 1, HI + 1))),
                              _spread(n - n_ge, list(range(L - 1, LO - 1, -1)))])
        X[:, i] = rng.permutation(col).astype(np.float32)
        Q[i, i] = scale
    return X, Q


def range_truth(S, tau):
    """S [nq, n] exact scores (any numeric dtype) -> lims int64 [nq + 1], ids int64, scores float32: per query the rows with
    S >= tau in the order np.lexsort((ids, -S)), i.e. (score desc, row asc)"""
    S = np.asarray(S)
    ids_all = np.arange(S.shape[1], dtype=np.int64)
    lims = np.zeros(S.shape[0] + 1, np.int64)
    ids, scores = [], []
    for i, row in enumerate(S):
        member = ids_all[row >= tau]
        member = member[np.lexsort((member, -row[member].astype(np.float64)))]
        ids.append(member)
        scores.append(row[member].astype(np.float32))
        lims[i + 1] = lims[i] + len(member)
    return lims, np.concatenate(ids) if ids else np.zeros(0, np.int64), \
        np.concatenate(scores) if scores else np.zeros(0, np.float32)


def filtered_truth(S, mask, k, row_offset=0):
    """S [nq, n] exact scores, mask bool [n] -> ids int64 [nq, k] (row_offset + row), scores float32 [nq, k]: the first k allowed
    rows in the order (score desc, row asc), padded with -1 / -inf"""
    S = np.asarray(S)
    mask = np.asarray(mask, bool)
    allowed = np.flatnonzero(mask).astype(np.int64)
    ids = np.full((S.shape[0], k), -1, np.int64)
    scores = np.full((S.shape[0], k), -np.inf, np.float32)
    for i, row in enumerate(S):
        order = allowed[np.lexsort((allowed, -row[allowed].astype(np.float64)))][:k]
        ids[i, :len(order)] = order + row_offset
        scores[i, :len(order)] = row[order].astype(np.float32)
    return ids, scores
