"""CPU: the dense float64 restatement of the per-node diffusion solve (oracle.diffusion_cg_dense / diffusion_solve_nodes),
which tests/test_gpu_diffusion_exact.py compares every device row with, pinned to scipy's cg and to the solutions the
reference's own get_offline_result recorded (tests/golden/diffusion_solve.npz); and the shape check of a cached offline
matrix in Diffusion.get_offline_results."""
import os

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import oracle
from isehr_amd.synth import synth_rows


def _golden_features():
    """The feature set of oracle/make_golden.py's diffusion fixtures (seeds 61 / 62: 300 clustered unit rows, 24-d)."""
    vd = synth_rows(61, 0, 300, 24).astype(np.float64)
    cd = synth_rows(62, 0, 12, 24).astype(np.float64)
    vd = 0.8 * vd + 1.1 * cd[np.arange(300) % 12]
    vd /= np.linalg.norm(vd, axis=1, keepdims=True)
    return vd.astype(np.float32)


# Both sides are float64 CG on the same matrix and differ in summation order only.  One dot product or matrix row of
# T = 200 terms is off by at most T * 2**-53 relative, carried through at most 20 iterations of a system whose condition
# number is below (1 + alpha) / (1 - alpha) = 199: 200 * 1.1e-16 * 20 * 199 < 1e-10 of the largest entry.  (Measured:
# 1.1e-15 absolute on entries up to 2.1.)  The issue's ceiling for this bound is 1e-9.
_REL = 1e-10


def test_dense_cg_matches_scipy_and_the_recorded_reference_solve(golden_dir):
    z = np.load(os.path.join(golden_dir, "diffusion_solve.npz"))
    T, kd, nodes = int(z["n_trunc"]), int(z["kd"]), z["nodes"]
    f = _golden_features()
    sims, ids = oracle.knn_flat_ip(f, f, T)
    assert np.array_equal(ids[nodes], z["ids"])
    xs, its, margins, lap = oracle.diffusion_solve_nodes(sims, ids, kd, nodes)
    big = np.abs(z["scores"]).max()
    err = np.abs(xs - z["scores"]).max()
    print("dense CG vs recorded reference solve: max |d| %.3e (largest entry %.3f)" % (err, big))
    assert big > 1.0 and err <= _REL * big, err
    b = np.zeros(T)
    b[0] = 1
    worst = 0.0
    for r, i in enumerate(nodes):
        x, _ = spla.cg(lap[ids[i]][:, ids[i]], b, rtol=1e-6, atol=0.0, maxiter=20)
        worst = max(worst, np.abs(x - xs[r]).max())
    print("dense CG vs scipy cg: max |d| %.3e" % worst)
    assert worst <= _REL * big, worst
    # both exits of the loop occur among the 50 nodes, and no residual sits on the threshold
    assert (its == 20).any() and (its < 20).any(), np.bincount(its)
    assert margins.min() > 1e-6, margins.min()


@pytest.mark.parametrize("alpha,gamma,maxiter,tol", [(0.5, 3, 20, 1e-6), (0.999, 1, 5, 1e-6), (0.99, 2, 200, 1e-10),
                                                     (0.99, 3, 1, 1e-6), (0.99, 3, 20, 1e-3)])
def test_dense_cg_matches_scipy_at_other_parameters(alpha, gamma, maxiter, tol):
    f = _golden_features()
    T, kd = 120, 30
    sims, ids = oracle.knn_flat_ip(f, f, T)
    nodes = np.arange(0, 300, 11)
    xs, its, margins, lap = oracle.diffusion_solve_nodes(sims, ids, kd, nodes, alpha, gamma, maxiter, tol)
    # get_laplacian(gamma=) reaches the affinity
    want = oracle.get_affinity(sims[:, :kd].copy(), ids[:, :kd], gamma)
    deg = np.asarray(want.sum(axis=1)).ravel()
    i = int(np.argmax(deg))
    j = int(want.tocsr()[i].indices[0])
    s_ij = float(want[i, j]) / np.sqrt((deg[i] + 1e-12) * (deg[j] + 1e-12))
    assert abs(float(lap[i, j]) + alpha * s_ij) < 1e-6
    b = np.zeros(T)
    b[0] = 1
    worst = 0.0
    for r, n in enumerate(nodes):
        x, _ = spla.cg(lap[ids[n]][:, ids[n]], b, rtol=tol, atol=0.0, maxiter=maxiter)
        worst = max(worst, np.abs(x - xs[r]).max())
    # up to 200 iterations here: the rounding bound grows with the iteration count
    assert worst <= _REL * max(1, maxiter / 20) * np.abs(xs).max(), worst


def test_dense_cg_trivial_systems():
    x, it, margin = oracle.diffusion_cg_dense(np.eye(5))
    assert np.array_equal(x, np.eye(5)[0]) and it == 1
    x, it, margin = oracle.diffusion_cg_dense(np.eye(5), maxiter=0)
    assert not x.any() and it == 0 and margin == np.inf


def _diffusion_without_device(n, cache_dir):
    from isehr_amd.diffusion import Diffusion
    d = Diffusion.__new__(Diffusion)           # the cache branch fails before it touches the device handle
    d.group, d.N, d.cache_dir, d.gallery, d.n_trunc = None, n, cache_dir, None, None
    return d


def test_cached_offline_matrix_must_fit_the_database(tmp_path):
    import joblib
    n, t = 6, 3
    cols = np.array([[(i + j) % n for j in range(t)] for i in range(n)])
    vals = np.arange(1, n * t + 1, dtype=np.float32).reshape(n, t)
    good = sp.csr_matrix((vals.ravel(), (np.repeat(np.arange(n), t), cols.ravel())), shape=(n, n), dtype=np.float32)
    path = str(tmp_path / "offline.jbl")
    # another database's cache
    joblib.dump(good, path)
    with pytest.raises(ValueError, match="shape"):
        _diffusion_without_device(n + 1, str(tmp_path)).get_offline_results(t, 2)
    # ragged rows: the entry count still divides by N, so a blind reshape would have gone through
    ragged_cols = [0, 1, 2, 3] + [1, 2] + [c for i in range(2, n) for c in cols[i]]
    ragged_rows = [0] * 4 + [1] * 2 + [i for i in range(2, n) for _ in range(t)]
    ragged = sp.csr_matrix((np.ones(n * t, dtype=np.float32), (ragged_rows, ragged_cols)), shape=(n, n))
    assert ragged.nnz == n * t
    joblib.dump(ragged, path)
    with pytest.raises(ValueError, match="per row"):
        _diffusion_without_device(n, str(tmp_path)).get_offline_results(t, 2)
    # zeros eliminated from one row
    holed = good.copy()
    holed.data[4] = 0
    holed.eliminate_zeros()
    joblib.dump(holed, path)
    with pytest.raises(ValueError, match="per row"):
        _diffusion_without_device(n, str(tmp_path)).get_offline_results(t, 2)
    # the well-formed matrix converts to the lists the device takes
    from isehr_amd.diffusion import _cached_lists
    ids, v = _cached_lists(good, n, path)
    assert ids.shape == (n, t) and ids.dtype == np.int64
    for i in range(n):
        assert dict(zip(ids[i].tolist(), v[i].tolist())) == dict(zip(cols[i].tolist(), vals[i].tolist()))
