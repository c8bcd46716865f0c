"""CPU: the scatter-matrix entry points answer their argument checks before any device is touched; the host-side
factorisation of whiten.py (eigh / Cholesky-with-jitter / ordering), fed a float64 numpy scatter matrix, reproduces the
reference's outputs recorded in tests/golden/whitenlearn.npz within 16 x the distance stored there between the reference and a
second correct float64 implementation (floor 1e-13); entry/learn_whitening's arguments and pickle format."""
import ctypes as C
import os
import pickle
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _whitenlearn_inputs as wi  # noqa: E402


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__
    __graft_entry__.build()
    from isehr_amd import _lib
    return _lib.load(), _lib


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "whitenlearn.npz")))


def test_scatter_entry_points_check_arguments_without_gpu(built_lib):
    lib, _lib = built_lib
    x = np.ones((4, 8), dtype=np.float32)
    out = np.zeros((8, 8))
    xp, op = C.c_void_p(x.ctypes.data), C.c_void_p(out.ctypes.data)
    q = np.array([0, 4], dtype=np.int64)
    p = np.array([1, 2], dtype=np.int64)
    qp, pp = C.c_void_p(q.ctypes.data), C.c_void_p(p.ctypes.data)
    b = C.c_int64(-1)

    def refused(rc, word):
        assert rc != 0 and word.encode() in lib.mi_last_error(), (rc, lib.mi_last_error())

    # workspace query: pure arithmetic
    assert lib.mi_scatter_workspace_bytes(2048, C.byref(b)) == 0 and b.value == 16 * 136 * 128 * 128 * 8
    assert lib.mi_scatter_workspace_bytes(11520, C.byref(b)) == 0 and 0 < b.value <= 512 << 20
    for d in (1, 24, 128, 129, 4096, 8192):
        assert lib.mi_scatter_workspace_bytes(d, C.byref(b)) == 0 and 0 < b.value <= 512 << 20
    refused(lib.mi_scatter_workspace_bytes(11521, C.byref(b)), "too large")
    refused(lib.mi_scatter_workspace_bytes(0, C.byref(b)), "bad sizes")
    refused(lib.mi_scatter_workspace_bytes(64, None), "null")
    # host entry point
    refused(lib.mi_scatter_matrix(None, 4, 8, 0, 8, 1, None, None, None, 0, 0, op), "null")
    refused(lib.mi_scatter_matrix(xp, 4, 8, 0, 8, 1, None, None, None, 0, 0, None), "null")
    refused(lib.mi_scatter_matrix(xp, 0, 8, 0, 8, 1, None, None, None, 0, 0, op), "bad sizes")
    refused(lib.mi_scatter_matrix(xp, 4, 8, 7, 8, 1, None, None, None, 0, 0, op), "dtype")
    refused(lib.mi_scatter_matrix(xp, 4, 8, 0, -8, 1, None, None, None, 0, 0, op), "negative strides")
    refused(lib.mi_scatter_matrix(xp, 4, 8, 0, 8, 1, None, qp, None, 2, 0, op), "together")
    refused(lib.mi_scatter_matrix(xp, 4, 8, 0, 8, 1, None, qp, pp, 0, 0, op), "n_pairs")
    refused(lib.mi_scatter_matrix(xp, 4, 8, 0, 8, 1, None, qp, pp, 2, 0, op), "pair index outside")
    refused(lib.mi_scatter_matrix(xp, 4, 20000, 0, 20000, 1, None, None, None, 0, 0, op), "too large")
    # device entry point: the same checks, then the workspace
    refused(lib.mi_scatter_matrix_device(None, 4, 8, 0, 8, 1, None, None, None, 0, op, 0, xp, 1 << 30, None), "null")
    refused(lib.mi_scatter_matrix_device(xp, 0, 8, 0, 8, 1, None, None, None, 0, op, 0, xp, 1 << 30, None), "bad sizes")
    refused(lib.mi_scatter_matrix_device(xp, 4, 20000, 0, 20000, 1, None, None, None, 0, op, 0, xp, 1 << 30, None), "too large")
    refused(lib.mi_scatter_matrix_device(xp, 4, 8, 0, 8, 1, None, None, None, 0, op, 0, None, 0, None), "workspace")
    refused(lib.mi_scatter_matrix_device(xp, 4, 8, 0, 8, 1, None, None, None, 0, op, 0, xp, 1024, None), "workspace smaller")
    refused(lib.mi_column_sum_device(None, 4, 8, 0, 8, 1, op, None), "null")
    # gallery entry point
    refused(lib.mi_gallery_scatter(None, None, op), "null")
    with pytest.raises(RuntimeError, match="too large"):
        _lib.scatter_workspace_bytes(20000)
    # the block-size option of the host entry point is plain state
    _lib.set_global_option("scatter_block_rows", 123)
    assert _lib.get_global_option("scatter_block_rows") == 123
    _lib.set_global_option("scatter_block_rows", 0)
    refused(lib.mi_set_global_option(b"scatter_block_rows", -1.0), "scatter_block_rows")


def _numpy_scatter(X, centre):
    Xc = np.asarray(X, dtype=np.float64) - np.asarray(centre, dtype=np.float64).reshape(-1, 1)
    return Xc @ Xc.T


@pytest.mark.parametrize("kind,dt", [(k, t) for k in wi.KINDS for t in ("f64", "f32")])
def test_host_factorisation_reproduces_the_reference(golden, kind, dt):
    from isehr_amd import whiten
    X64, q, p = wi.make_input(kind, int(golden["seed"]))
    X = wi.as_dtype(X64, dt).astype(np.float64)
    pre = "%s_%s_" % (kind, dt)
    m1 = X.mean(axis=1, keepdims=True)
    P1, ev = whiten.pca_from_scatter(_numpy_scatter(X, m1), X.shape[1])
    assert np.all(np.diff(ev) <= 0)                         # descending
    m2 = X[:, q].mean(axis=1, keepdims=True)
    df = X[:, q] - X[:, p]
    P2 = whiten.supervised_from_scatter(df @ df.T / q.size, _numpy_scatter(X, m2))
    for tag, m, P in (("pca", m1, P1), ("sup", m2, P2)):
        m_ref, P_ref = golden[pre + "m_" + tag], golden[pre + "P_" + tag]
        assert np.max(np.abs(m - m_ref)) <= 4 * X.shape[1] * wi.U * np.max(np.abs(X))
        dr, dg = wi.rows_distance(P, P_ref), wi.gram_distance(P, P_ref)
        print("%s %s %s: rows %.3e (stored %.3e), P.T P %.3e (stored %.3e)" %
              (kind, dt, tag, dr, float(golden[pre + "dev_rows_" + tag]), dg, float(golden[pre + "dev_gram_" + tag])))
        assert dr <= max(16 * float(golden[pre + "dev_rows_" + tag]), 1e-13)
        assert dg <= max(16 * float(golden[pre + "dev_gram_" + tag]), 1e-13)
    # what the result is for: P Xcov P^T = I
    W = P1 @ (_numpy_scatter(X, m1) / X.shape[1]) @ P1.T
    assert np.max(np.abs(W - np.eye(wi.D))) <= 64 * (ev[0] / ev[-1]) * wi.D * wi.U


def test_fixture_meets_its_conditions(golden):
    assert int(golden["D"]) == wi.D and int(golden["N"]) == wi.N and int(golden["N_PAIRS"]) == wi.N_PAIRS
    for kind in wi.KINDS:
        for dt in ("f64", "f32"):
            assert float(golden["%s_%s_min_gap" % (kind, dt)]) >= 1e-3
            assert golden["%s_%s_P_pca" % (kind, dt)].dtype == np.float64


def test_rank_deficient_and_jitter():
    from isehr_amd import whiten
    rng = np.random.default_rng(1)
    A = rng.standard_normal((12, 5))
    with pytest.raises(ValueError, match="7 of 12 eigenvalues"):
        whiten.pca_from_scatter(A @ A.T, 5)
    S = A[:, :3] @ A[:, :3].T                                  # rank 3: not positive definite
    L, alpha = whiten.cholesky_jitter(S)
    assert alpha > 0 and np.log10(alpha) == pytest.approx(round(np.log10(alpha))) and alpha >= 1e-10
    assert np.allclose(L @ L.T, S + alpha * np.eye(12), atol=1e-12)
    L0, a0 = whiten.cholesky_jitter(S + np.eye(12))
    assert a0 == 0.0
    B = rng.standard_normal((12, 200))
    P = whiten.supervised_from_scatter(S / 3, B @ B.T)
    assert P.shape == (12, 12) and np.all(np.isfinite(P))
    with pytest.raises(ValueError, match="pair index"):
        whiten._pairs([0, 5], [1, 2], 5)
    with pytest.raises(ValueError, match="one length"):
        whiten._pairs([0, 1], [1], 5)


def test_learn_whitening_driver_arguments_and_pickle(tmp_path, monkeypatch, capsys):
    """The driver with the device calls replaced by numpy: argument parsing, the three feature formats, the pickle."""
    from isehr_amd import _lib, whiten
    from isehr_amd.entry import learn_whitening
    from isehr_amd.entry.features import save_path_feature
    calls = []

    def np_scatter(rows, centre=None, pairs=None, device=0):
        calls.append("pairs" if pairs is not None else "rows")
        r = np.asarray(rows, dtype=np.float64)
        if pairs is not None:
            df = r[pairs[0]] - r[pairs[1]]
            return df.T @ df
        rc = r - (0.0 if centre is None else np.asarray(centre).reshape(1, -1))
        return rc.T @ rc

    monkeypatch.setattr(_lib, "scatter_matrix", np_scatter)
    monkeypatch.setattr(_lib, "column_sum", lambda rows, device=0: np.asarray(rows, dtype=np.float64).sum(axis=0))
    monkeypatch.chdir(tmp_path)
    X64, q, p = wi.make_input("graded", 11)
    X = X64.astype(np.float32)
    np.save("vecs.npy", X)
    with open("db.pkl", "wb") as f:
        pickle.dump({"qidxs": q.tolist(), "pidxs": p.tolist()}, f)
    assert learn_whitening.main(["--features", "vecs.npy", "--out", "Lw.pkl"]) == 0
    assert calls == ["rows"]
    with open("Lw.pkl", "rb") as f:
        Lw = pickle.load(f)
    assert sorted(Lw) == ["P", "m"] and Lw["m"].shape == (wi.D, 1) and Lw["P"].shape == (wi.D, wi.D)
    assert Lw["m"].dtype == np.float64 and Lw["P"].dtype == np.float64
    Xd = X.astype(np.float64)
    P_want, _ = whiten.pca_from_scatter(_numpy_scatter(Xd, Xd.mean(axis=1)), wi.N)
    assert wi.gram_distance(Lw["P"], P_want) <= 1e-10
    out = capsys.readouterr().out
    assert "PCA whitening of 3000 descriptors x 64 dimensions" in out and "scatter" in out and "factorisation" in out
    # supervised, from a feature-store pickle
    save_path_feature("ds", X, ["im%d" % i for i in range(wi.N)])
    del calls[:]
    assert learn_whitening.main(["--features", "outputs/features/ds_path_feature.pkl", "--pairs", "db.pkl", "-o", "Lw2.pkl"]) == 0
    assert calls == ["pairs", "rows"] and "supervised" in capsys.readouterr().out
    with open("Lw2.pkl", "rb") as f:
        Lw2 = pickle.load(f)
    assert np.array_equal(Lw2["m"], Xd[:, q].mean(axis=1, keepdims=True)) and np.all(np.isfinite(Lw2["P"]))
    # refused combinations
    for argv in (["--out", "x.pkl"], ["--features", "vecs.npy", "--gallery", "g.gal", "--out", "x.pkl"],
                 ["--gallery", "g.gal", "--pairs", "db.pkl", "--out", "x.pkl"], ["--features", "vecs.npy"]):
        with pytest.raises(SystemExit):
            learn_whitening.main(argv)
    with open("bad.pkl", "wb") as f:
        pickle.dump({"qidxs": [0]}, f)
    with pytest.raises(ValueError, match="qidxs"):
        learn_whitening.main(["--features", "vecs.npy", "--pairs", "bad.pkl", "--out", "x.pkl"])
