"""CPU: k-means over whole rows (mi_kmeans_*).  Argument limits raise ValueError before the library loads; KMeans
refuses predict before fit; the numpy restatement of the certificate (tests/_kmeans_truth.py: tau_rows) is what its derivation
says -- on integer data both forms are exact, and on float data the errors measured against exact rational arithmetic stay within
the quarter of tau each form is allowed."""
from fractions import Fraction

import numpy as np
import pytest

from _kmeans_truth import U, assign_truth, expanded_gap, gamma, lattice, near_ties, tau_rows
from _pq_train_truth import clustered


@pytest.fixture()
def lib(monkeypatch):
    from isehr_amd import _lib

    def no_load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_load)
    return _lib


X = np.random.RandomState(0).randn(40, 8).astype(np.float32)


@pytest.mark.parametrize("k", [-1, 0, 1, 8193, 1 << 20])
def test_k_outside_its_range(lib, k):
    big = np.zeros((max(k, 2), 2), np.float32)
    with pytest.raises(ValueError):
        lib.kmeans_train(big, k)
    with pytest.raises(ValueError):
        lib.kmeans_train_device(0, big.shape[0], 2, k, 3)
    with pytest.raises(ValueError):
        lib.KMeans(k)
    with pytest.raises(ValueError):
        lib.kmeans_assign(X, np.zeros((max(k, 0), 8), np.float32))
    with pytest.raises(ValueError):
        lib.IVFFlatIndex.train_matrix(big, k)


def test_shape_and_iteration_limits(lib):
    with pytest.raises(ValueError):
        lib.kmeans_train(X, 41)                                   # n < k
    with pytest.raises(ValueError):
        lib.kmeans_train_device(0, 40, 8, 41, 3)
    for iters in (0, -3):
        with pytest.raises(ValueError):
            lib.kmeans_train(X, 4, iters=iters)
        with pytest.raises(ValueError):
            lib.KMeans(4, iters=iters)
    with pytest.raises(ValueError):
        lib.kmeans_train(np.zeros((10, 4097), np.float32), 4)     # d > 4096
    with pytest.raises(ValueError):
        lib.kmeans_train(X[0], 4)                                 # not 2-D


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_rows_and_centroids(lib, bad):
    x = X.copy()
    x[17, 3] = bad
    with pytest.raises(ValueError):
        lib.kmeans_train(x, 4)
    with pytest.raises(ValueError):
        lib.kmeans_assign(x, X[:4])
    with pytest.raises(ValueError):
        lib.kmeans_assign(X, x[16:20])
    with pytest.raises(ValueError):
        lib.kmeans_train(X, 4, init=x[16:20])


def test_one_initialisation_at_most(lib):
    init, rows = X[:4], np.arange(4)
    for kw in (dict(init=init, init_rows=rows), dict(init=init, seed=1), dict(init_rows=rows, seed=1),
               dict(init=init, init_rows=rows, seed=1)):
        with pytest.raises(ValueError):
            lib.kmeans_train(X, 4, **kw)
    with pytest.raises(ValueError):
        lib.kmeans_train(X, 4, init=X[:5])                        # [k, d] it must be
    with pytest.raises(ValueError):
        lib.kmeans_train(X, 4, init_rows=np.array([0, 1, 2, 40]))  # a row that does not exist
    with pytest.raises(ValueError):
        lib.kmeans_train(X, 4, init_rows=np.array([0.0, 1.0, 2.0, 3.0]))


def test_train_matrix_takes_what_train_takes(lib):
    """IVFFlatIndex.train keeps its parameter list (tests/test_ivfflat_cpu.py pins it), so the matrix path is a method beside it
    with the same parameters and defaults, not a keyword; an engine keyword is refused like any unknown one."""
    import inspect
    a, b = inspect.signature(lib.IVFFlatIndex.train), inspect.signature(lib.IVFFlatIndex.train_matrix)
    assert a.parameters.keys() == b.parameters.keys() and all(a.parameters[k].default == b.parameters[k].default for k in a.parameters)
    with pytest.raises(TypeError):
        lib.IVFFlatIndex.train(X, 4, engine="matrix")


def test_predict_before_fit(lib):
    km = lib.KMeans(4)
    assert km.cluster_centers_ is None and km.labels_ is None and km.n_iter_ is None
    with pytest.raises(ValueError):
        km.predict(X)


# ---- the certificate
def test_tau_on_integer_data_where_both_forms_are_exact():
    """lattice data: every product and every partial sum is a small integer, so float64 evaluates both forms without error -- the
    measured error is 0, the forms agree and tau, which must be positive, is 4 gamma (||x|| + cmax)^2 of the exact norms."""
    x, C = lattice(np.random.RandomState(1), 200, 30)
    xi, Ci = x.astype(np.int64), C.astype(np.int64)
    direct = ((xi[:, None, :] - Ci[None]) ** 2).sum(-1)                          # exact integers
    e_exact = (Ci * Ci).sum(1)[None] - 2 * (xi @ Ci.T)
    x64, C64 = x.astype(np.float64), C.astype(np.float64)
    acc = np.zeros(direct.shape)
    for j in range(x.shape[1]):
        acc += (x64[:, None, j] - C64[None, :, j]) ** 2
    assert np.array_equal(acc, direct)                                           # error 0
    assert np.array_equal((C64 * C64).sum(1)[None] - 2.0 * (x64 @ C64.T), e_exact)
    assert np.array_equal(direct - (xi * xi).sum(1)[:, None], e_exact)
    tau = tau_rows(x, C)
    want = 4 * gamma(17) * (np.sqrt((xi * xi).sum(1)) + np.sqrt((Ci * Ci).sum(1).max())) ** 2
    assert (tau > want).all() and (tau < want * (1 + 1e-8) + 1e-290).all()
    ties = (np.sort(direct, 1)[:, 0] == np.sort(direct, 1)[:, 1]).sum()
    assert ties >= 10                                                            # the input the fallback test needs
    assert (expanded_gap(x, C)[np.sort(direct, 1)[:, 0] == np.sort(direct, 1)[:, 1]] == 0).all()


@pytest.mark.parametrize("d,shift", [(1, 0.0), (17, 0.0), (33, 100.0), (64, 1e6)])
def test_tau_bounds_the_measured_error_of_both_forms(d, shift):
    """float data, errors measured against exact rational arithmetic: |direct - D| <= tau / 4 and |expanded - (||c||^2 - 2 x.c)|
    <= tau / 4 for every (row, centroid), the direct form summed in ascending j and the expanded form both in ascending j and in
    numpy's own order."""
    rng = np.random.RandomState(d)
    x = (rng.randn(6, d) * 3 + shift).astype(np.float32 if shift < 1e6 else np.float64)
    C = (rng.randn(5, d) * 3 + shift).astype(np.float32)
    x64, C64 = x.astype(np.float64), C.astype(np.float64)
    tau = tau_rows(x, C)
    cn_np = (C64 * C64).sum(1)
    dots_np = x64 @ C64.T
    worst = 0.0
    for i in range(x.shape[0]):
        for c in range(C.shape[0]):
            fx, fc = [Fraction(float(v)) for v in x64[i]], [Fraction(float(v)) for v in C64[c]]
            D = sum((a - b) ** 2 for a, b in zip(fx, fc))
            e = sum(b * b for b in fc) - 2 * sum(a * b for a, b in zip(fx, fc))
            acc, cn, dot = 0.0, 0.0, 0.0
            for j in range(d):
                t = x64[i, j] - C64[c, j]
                acc = acc + t * t
                cn = cn + C64[c, j] * C64[c, j]
                dot = dot + x64[i, j] * C64[c, j]
            errs = [abs(Fraction(float(acc)) - D), abs(Fraction(float(cn - 2.0 * dot)) - e),
                    abs(Fraction(float(cn_np[c] - 2.0 * dots_np[i, c])) - e)]
            for err in errs:
                assert err <= Fraction(float(tau[i])) / 4, (i, c, float(err), tau[i])
                worst = max(worst, float(err) / tau[i])
    assert worst < 0.25


def test_the_continuous_inputs_leave_the_certificate_room():
    """the inputs of the GPU test 'the MFMA path must carry the result': the smallest gap between the two best expanded values is
    far above tau, with all data shifted by +100 as well, so the expected flagged count is 0."""
    for (n, k, d) in [(300, 130, 64), (257, 129, 17), (300, 130, 33), (129, 2, 1)]:
        for seed in range(3):
            x, _ = clustered(np.random.RandomState(seed), n, 1, k, d)
            C = x[(np.arange(k) * n) // k]
            for xs, Cs in ((x, C), (x + np.float32(100), C + np.float32(100))):
                gap, tau = expanded_gap(xs, Cs), tau_rows(xs, Cs)
                assert gap.min() >= 1.4e-3 and tau.max() <= 7.5e-5, (n, k, d, seed, gap.min(), tau.max())


def test_near_tie_rows_straddle_the_bound():
    """the k = 2 input of the GPU near-tie test: the expanded gap of the rows displaced by s * tau is about s * tau, on both sides
    of the bound, and the direct-form truth puts the displaced rows on the side they were moved to."""
    x, C = near_ties()
    tau = tau_rows(x, C)
    gap = expanded_gap(x, C)
    s = np.repeat([0.0, 1e-3, 0.5, 2.0, 1e3], 2)
    assert (gap[s <= 0.5] <= tau[s <= 0.5]).all() and (gap[s == 1e3] > tau[s == 1e3]).all()
    ids = assign_truth(x, C)
    assert np.array_equal(ids[s >= 2.0], np.tile([0, 1], 2))      # side -1 is towards centroid 0
    assert U == 2.0 ** -53
